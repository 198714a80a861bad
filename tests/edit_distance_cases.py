"""TEST INFRASTRUCTURE of tests/test_edit_distance_emu.py and tests/test_gpu_edit_distance.py: a fixed, seeded table of cases
through edit_distance_batch_raw (numpy: fcd_edit_distance_host; torch: fcd_duplex_envelope_dev under fcd_set_edit_distance)
against `reference`, a numpy int64 row-by-row DP of the definition in include/fcd.h.  Integer work: every comparison is
exact equality on distance and end."""
import ctypes as C

import numpy as np
import pytest

TIERS = (0, 1, 63, 64, 65, 128, 129, 257, 511, 512, 513, 1024, 1025)  # len(b): every W, the carries between blocks, g = 2, 4
GROUPS = (4097, 8193, 32768)  # g = 16 (the last tier inside a DPP row), 32 (crosses rows), 64
CASES = {
    **{"tier_L%d_A%d" % (L, A): dict(len2=[L] * 3, len1=[max(L - 3, 0), L, L + 2], A=A) for L in TIERS for A in (5, 16)},
    **{"group_L%d" % L: dict(len2=[L] * 3, len1=[0, 1, 70], A=16, mutate=False) for L in GROUPS},
    "content": dict(content=True),
    **{"batch_n%d" % n: dict(n=n) for n in (1, 64, 65, 130)},
    "no_value": dict(n=8, no_value=True),
    "result_method": dict(result=True),
    "one_pair_and_refusals": dict(refusals=True),
}


def reference(a, b, mode):
    """-> (distance, end): rows over a, D[i][j] of a[s:i] against b[:j]; the in-row term D[i][j-1] + 1 as a running minimum"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    j = np.arange(len(b) + 1, dtype=np.int64)
    row, best, end = j.copy(), len(b), 0
    for i in range(1, len(a) + 1):
        cand = np.empty_like(row)
        cand[0] = i if mode == "global" else 0
        cand[1:] = np.minimum(row[1:] + 1, row[:-1] + (b != a[i - 1]))
        row = np.minimum.accumulate(cand - j) + j
        if row[-1] < best:
            best, end = int(row[-1]), i
    return (int(row[-1]), len(a)) if mode == "global" else (best, end)


def _mutated(rng, b, n, A):
    """n labels: b with about a tenth of its labels substituted, dropped or doubled, cut or padded to n"""
    out = []
    for v in b:
        u = rng.random()
        out += [] if u < 0.03 else [v, v] if u < 0.06 else [int(rng.integers(1, A))] if u < 0.1 else [v]
    out = out[:n] + list(rng.integers(1, A, max(n - len(out), 0)))
    return np.asarray(out, np.uint8)


def build(name):
    """-> (labels1 (n, cap1), len1, labels2 (n, cap2), len2): views of arrays three columns wider (strides cap + 3)"""
    k, rng = CASES[name], np.random.default_rng(sorted(CASES).index(name))
    A = k.get("A", 5)
    if k.get("content"):
        x, hom = rng.integers(1, 5, 300).astype(np.uint8), np.full(90, 2, np.uint8)
        planted = np.delete(x[100:180], 40)
        planted[10] = planted[10] % 4 + 1  # two edits; the reference's smallest-e rule places the end
        pairs = [(x, x), (x[:70] % 2 + 1, x[:90] % 2 + 3), (hom, hom[:60]), (hom[:60], hom), (x[:40], x), (x, planted)]
    elif "n" in k:  # ragged inside one wavefront, zero lengths, more than one block
        n = k["n"]
        l1, l2 = rng.integers(0, 150, n), rng.integers(0, 150, n)
        l1[::7], l2[3::11] = 0, 0
        pairs = []
        for i in range(n):
            b = rng.integers(1, A, l2[i]).astype(np.uint8)
            pairs.append((_mutated(rng, b, l1[i], A), b))
    else:
        pairs = []
        for n1, n2 in zip(k["len1"], k["len2"]):
            b = rng.integers(1, A, n2).astype(np.uint8)
            pairs.append((_mutated(rng, b, n1, A) if k.get("mutate", True) else rng.integers(1, A, n1).astype(np.uint8), b))
    n = len(pairs)
    out = []
    for s in (0, 1):
        lens = np.array([len(p[s]) for p in pairs], np.uint32)
        cap = max(int(lens.max()) - (20 if "n" in k else 0), 1)  # (batch cases: caps below the longest lengths clip)
        wide = np.zeros((n, cap + 3), np.uint8)
        for i, p in enumerate(pairs):
            wide[i, :min(len(p[s]), cap)] = p[s][:cap]
        out += [wide[:, :cap], lens]
    if k.get("no_value"):
        (a, l1, b, l2) = out
        l1[:6], l2[:6] = np.minimum(l1[:6], 100), np.minimum(l2[:6], 100)
        a[0, l1[0]:] = 16    # beyond the length: changes nothing
        b[1, l2[1]:] = 255
        a[3, max(min(int(l1[3]), a.shape[1]) - 1, 0)], l1[3] = 16, max(l1[3], 1)  # inside: no value for this pair alone
        b[5, 0], l2[5] = 200, max(l2[5], 1)
    return out


def check(got, arrays, mode, where):
    a, l1, b, l2 = arrays
    dist, end = (np.asarray(v.cpu() if hasattr(v, "cpu") else v) for v in got)
    assert dist.dtype == np.int32 and end.dtype == np.int32
    for r in range(len(l1)):
        x, y = a[r, :min(int(l1[r]), a.shape[1])], b[r, :min(int(l2[r]), b.shape[1])]
        want = (-1, -1) if max(x.max(initial=0), y.max(initial=0)) >= 16 else reference(x, y, mode)
        assert (int(dist[r]), int(end[r])) == want, (where, mode, r, len(x), len(y), int(dist[r]), int(end[r]), want)


def run_case(fcd, name, device=None):
    k = CASES[name]
    to = (lambda v: v) if device is None else (lambda v: __import__("torch").from_numpy(np.ascontiguousarray(v)).to(device))
    if k.get("refusals"):
        assert fcd.edit_distance("ACGT", "AGT") == 1 and fcd.edit_distance("TTACGTT", "AGT", mode="infix") == 1
        one, n1 = np.ones((1, 4), np.uint8), np.array([4], np.uint32)
        with pytest.raises(ValueError, match="mode"):
            fcd.edit_distance_batch_raw(one, n1, one, n1, mode="local")
        from fast_ctc_decode_amd import _native as nat
        h, ptr = nat.default_handle(), (one.ctypes.data, n1.ctypes.data)
        for stride, out in ((4, nat.EditDistance(None, None, 0)), (3, nat.EditDistance(n1.ctypes.data, None, 0)), (4, nat.EditDistance(n1.ctypes.data, None, 2))):
            assert h.lib.fcd_edit_distance_host(h.ptr, 1, *ptr, stride, 4, *ptr, 4, 4, C.byref(out)) == nat.E_INVALID, stride
        assert n1[0] == 4  # (nothing was written)
        with pytest.raises(RuntimeError, match="32768"):
            fcd.edit_distance_batch_raw(to(one), to(n1), to(np.ones((1, 32769), np.uint8)), to(n1))
        return
    if k.get("result"):  # the result's own labels are sequence 2, found inside a longer truth in infix mode
        x = np.random.default_rng(5).random((5, 90, 5), np.float32)
        res = fcd.viterbi_search_batch_raw(to(x / x.sum(-1, keepdims=True)))
        host = res.cpu()
        truth = np.concatenate([np.full((5, 4), 2, np.uint8), host.labels[:, :60], np.full((5, 6), 3, np.uint8)], 1)
        for mode in ("global", "infix"):
            got = res.edit_distance(truth, np.full(5, 70, np.uint32), mode, return_end=True)
            assert type(got[0]) is type(res.out_len)
            check(got, (truth, np.full(5, 70), host.labels, host.out_len), mode, name)
        return
    arrays = build(name)
    for mode in ("global", "infix"):
        a, l1, b, l2 = arrays
        if device is None:
            got = fcd.edit_distance_batch_raw(a, l1, b, l2, mode, return_end=True)
        else:  # (views of the wider device arrays: the strides stay cap + 3)
            got = fcd.edit_distance_batch_raw(to(a.base)[:, :a.shape[1]], to(l1.view(np.int32)), to(b.base)[:, :b.shape[1]],
                                              to(l2.view(np.int32)), mode, return_end=True)
        check(got, arrays, mode, name)
        if device is None:
            assert np.array_equal(fcd.edit_distance_batch_raw(a, l1, b, l2, mode), got[0])
