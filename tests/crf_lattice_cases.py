"""TEST INFRASTRUCTURE shared by tests/test_crf_lattice_emu.py (the kernels on the wave64 emulator) and
tests/test_gpu_crf_lattice.py (on the GPU): seeded cases run through crf_score_batch_raw / crf_align_batch_raw and compared
with the restatement tests/crf_lattice_reference.py, and the greedy-parity check against crf_greedy_search.

start, count and qual must equal the restatement EXACTLY (the kernel's arithmetic is the restatement's: f32 mantissa
products, exact rescaling, the same tie rule); align's logp within 1e-12 relative (ctc_align_cases.logp_same); the score
within 4 T_r 2^-24 nats of the float64 restatement (three f32 roundings per cell and row, non-negative terms).
Condition on the inputs, asserted for every labelling: the restatement with drop=2^-160 returns the same alignment -- no
case relies on cells the contract lets the kernel drop.
Properties: emission rows strictly ascending and below T_r; the float64 product along the returned alignment is logp
within 2 T_r 2^-24; align logp <= score; band W <= band 2W <= exact, for the score (each side within its tolerance) and
for align's logp (no slack beyond logp_same: max and a single rounding are monotone, the rescaling is exact).

A case: (name, S, N, T, B, n_hyp, dtype, layout, bands, fill) -- fill: labels per row of the read, roughly."""
import math

import numpy as np

import crf_lattice_reference as R
from ctc_align_cases import logp_same


def tolerance(Tr):
    return 4 * max(Tr, 1) * 2.0 ** -24


def posteriors(rng, B, T, S, N, sharp=1.0):
    x = rng.random((B, T, S, N)) ** (1.0 + 2.0 * sharp)
    x[..., 0] *= 1.5
    return (x / x.sum(-1, keepdims=True)).astype(np.float32)


# exact mode and the bands 1 / 4 / 31 / 32 / 64 / 128: windows of 3, 9, 63 (K = 1), 65 (K = 2), 129 (K = 4), 257 (K = 8)
# states; exact windows of T + 1 states.  S * N = 20 gives tiles of 51 rows: T = 51, 52 are its edges.  S * N = 1020 is
# the last staged shape (one row a tile), 1025 and 5120 are gathered from global memory.  "wrap" cases: more labels than
# the K's slots, so that the window travels round the ring.
CASES = [
    ("s4n5_t1", 4, 5, 1, 3, 1, "f32", "read", (0, 1), 0.5),
    ("s4n5_t9_f16", 4, 5, 9, 3, 2, "f16", "read", (0, 1, 4), 0.6),
    ("s4n5_t51", 4, 5, 51, 2, 1, "f32", "read", (0, 4), 0.7),
    ("s4n5_t52_tm", 4, 5, 52, 3, 3, "f32", "time", (0, 4, 31), 0.7),
    ("s16n5_t64_bf16", 16, 5, 64, 2, 1, "bf16", "read", (0, 32), 0.8),
    ("s16n5_t65", 16, 5, 65, 2, 5, "f32", "read", (0, 1, 32), 0.8),
    ("s64n5_t200", 64, 5, 200, 2, 2, "f32", "read", (0, 31, 32, 64), 0.75),
    ("s4n5_t300", 4, 5, 300, 2, 1, "f16", "time", (0, 64, 128), 0.9),
    ("s1024n5_t65_f16_tm", 1024, 5, 65, 2, 2, "f16", "time", (0, 4), 0.7),
    ("s204n5_t9", 204, 5, 9, 2, 1, "f32", "read", (0, 1), 0.6),
    ("s205n5_t9", 205, 5, 9, 2, 1, "f32", "read", (0, 1), 0.6),
    ("s5n4_t52", 5, 4, 52, 3, 2, "f32", "read", (0, 4), 0.2),
    ("s6n3_t64", 6, 3, 64, 2, 1, "f32", "read", (0, 4, 32), 0.7),
    ("s6n2_t51", 6, 2, 51, 2, 2, "f32", "read", (0, 4), 0.5),
    ("s1n4_t9", 1, 4, 9, 2, 1, "f32", "read", (0, 1), 0.4),
    ("wrap_k1_s4n5_t200", 4, 5, 200, 1, 1, "f32", "read", (1, 4), 0.8),
    ("wrap_k2_s16n5_t200", 16, 5, 200, 1, 1, "f32", "read", (32,), 0.9),
    ("wrap_k4_s4n5_t300", 4, 5, 300, 1, 1, "f32", "read", (64,), 0.95),
    ("wrap_k8_s4n5_t1100", 4, 5, 1100, 1, 1, "f32", "read", (128,), 0.55),
]
# the slice of the grid the GPU twin runs: one case per K, both staging regimes, f16, time-major
GPU_CASES = ("s4n5_t52_tm", "s16n5_t65", "s64n5_t200", "s4n5_t300", "s1024n5_t65_f16_tm", "s205n5_t9", "s5n4_t52",
             "wrap_k8_s4n5_t1100")


def build_case(case):
    name, S, N, T, B, n_hyp, dtype, layout, bands, fill = case
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    x = posteriors(rng, B, T, S, N)
    if dtype == "f16":
        xin = x.astype(np.float16)
        x32 = xin.astype(np.float32)
    elif dtype == "bf16":
        bits = (x.view(np.uint32) >> 16).astype(np.uint16)  # truncation: any bf16 value will do
        xin, x32 = bits, (bits.astype(np.uint32) << 16).view(np.float32)
    else:
        xin = x32 = x
    if layout == "time":
        xin = np.ascontiguousarray(xin.transpose(1, 0, 2, 3)).transpose(1, 0, 2, 3)
    lengths = None
    if B > 1:
        lengths = rng.integers(max(1, T // 2), T + 1, size=B).astype(np.int64)
        lengths[0] = T
    init = rng.random((B, S + (1 if name.startswith("s5n4") else 0))).astype(np.float32)
    labels = np.zeros((B, n_hyp, T), np.uint8)
    paths = np.zeros((B, n_hyp, T), np.uint32)
    out_len = np.zeros((B, n_hyp), np.uint32)
    for b in range(B):
        Tr = T if lengths is None else int(lengths[b])
        for i in range(n_hyp):
            L = min(Tr, int(round(fill * Tr * (1.0 - 0.1 * i))))
            rows = np.sort(rng.choice(Tr, L, replace=False))
            labels[b, i, :L] = rng.integers(1, N, L)
            paths[b, i, :L] = rows
            out_len[b, i] = L
    n_valid = None
    if n_hyp > 1:
        n_valid = rng.integers(1, n_hyp + 1, size=B).astype(np.uint32)
        n_valid[0] = n_hyp
    return dict(name=name, S=S, N=N, T=T, B=B, n_hyp=n_hyp, dtype=dtype, xin=xin, x32=x32, init=init, lengths=lengths,
                labels=labels, paths=paths, out_len=out_len, n_valid=n_valid, bands=bands)


def check(got, score, x32, init, lengths, labels, paths, out_len, n_valid, band, rows=None):
    """got: AlignResult of numpy arrays, score: (B, n_hyp) float64 or None; x32: the posteriors as float32 (the exact
    upcast of what the kernel read).  -> {(b, i): (restatement alignment, restatement score)}"""
    B, n_hyp = got.logp.shape
    refs = {}
    for b in (range(B) if rows is None else rows):
        Tr = x32.shape[1] if lengths is None else int(lengths[b])
        for i in range(n_hyp):
            n = int(out_len[b, i])
            if n_valid is not None and i >= int(n_valid[b]):
                assert got.logp[b, i] != got.logp[b, i], ("rows that are no hypothesis are NaN", b, i)
                assert score is None or score[b, i] != score[b, i]
                assert (got.count[b, i, :min(n, labels.shape[2])] == 0).all()
                continue
            y, pth = labels[b, i, :n], (paths[b, i, :n] if band else None)
            ref = R.crf_align(x32[b, :Tr], init[b], y, band, pth)
            cond = R.crf_align(x32[b, :Tr], init[b], y, band, pth, drop=2.0 ** -160)
            assert ref["start"] == cond["start"], ("the case relies on dropped cells", b, i)
            where = (b, i, "T_r", Tr, "L", n, "band", band)
            print("align", where, got.logp[b, i], ref["logp"])
            assert logp_same(got.logp[b, i], ref["logp"]), where + (got.logp[b, i], ref["logp"])
            want = None
            if score is not None:
                want = R.crf_score(x32[b, :Tr], init[b], y, band, pth)
                print("score", where, score[b, i], want, tolerance(Tr))
                if want != want or math.isinf(want):
                    assert logp_same(score[b, i], want), where + (score[b, i], want)
                else:
                    assert abs(score[b, i] - want) <= tolerance(Tr), where + (score[b, i], want)
                    if got.logp[b, i] == got.logp[b, i]:  # one alignment is no more than all of them
                        assert got.logp[b, i] <= score[b, i] + tolerance(Tr), where + (got.logp[b, i], score[b, i])
            refs[(b, i)] = (ref, want)
            if ref["start"] is None:
                assert (got.count[b, i, :n] == 0).all(), where
                continue
            assert got.start[b, i, :n].tolist() == ref["start"], where
            assert got.count[b, i, :n].tolist() == ref["count"], where
            assert got.qual[b, i, :n].view(np.uint32).tolist() == np.asarray(ref["qual"], np.float32).view(np.uint32).tolist(), where
            st = got.start[b, i, :n].astype(np.int64)
            assert (st[1:] > st[:-1]).all() and (n == 0 or st[-1] < Tr), where
            sig = R.trajectory(init[b], y, x32.shape[2], x32.shape[3])
            prod, k = 0.0, 0
            for t in range(Tr):
                if k < n and st[k] == t:
                    prod += math.log(float(x32[b, t, sig[k], y[k]]))
                    k += 1
                else:
                    prod += math.log(float(x32[b, t, sig[k], 0]))
            assert abs(prod - got.logp[b, i]) <= 2 * Tr * 2.0 ** -24, where + (prod, got.logp[b, i])
    return refs


def _device_inputs(c, device):
    kw = {}
    if device is None:
        if c["dtype"] == "bf16":
            kw["input_dtype"] = "bfloat16"
        return c["xin"], (lambda a: a), kw
    import torch
    if c["dtype"] == "bf16":
        xin = torch.from_numpy(np.ascontiguousarray(c["xin"]).view(np.int16)).to(device).view(torch.bfloat16)
    else:
        xin = torch.from_numpy(np.ascontiguousarray(c["xin"])).to(device)
    if c["xin"].strides[0] < c["xin"].strides[1]:  # time-major on the device too
        xin = xin.transpose(0, 1).contiguous().transpose(0, 1)
    conv = lambda a: None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device)
    return xin, conv, kw


def run_case(fcd, c, device=None):
    """scores and aligns the case at each of its bands, checks every labelling against the restatement, then the
    properties that tie the bands to one another"""
    xin, conv, kw = _device_inputs(c, device)
    by_band = {}
    for band in c["bands"]:
        args = (xin, conv(c["init"]), conv(c["labels"]), conv(c["out_len"]), conv(c["lengths"]),
                conv(c["paths"]) if band else None, band, conv(c["n_valid"]))
        got = fcd.crf_align_batch_raw(*args, **kw)
        score = fcd.crf_score_batch_raw(*args, **kw)
        if device is not None:
            import torch
            assert got.start.device == xin.device and got.logp.dtype == torch.float64 and score.dtype == torch.float64
            score = score.cpu().numpy()
        got = got.cpu()
        assert got.start.shape == c["labels"].shape and got.count.shape == c["labels"].shape
        assert got.qual.shape == c["labels"].shape and got.logp.shape == c["out_len"].shape == score.shape
        assert got.start.dtype == np.uint32 and got.qual.dtype == np.float32 and got.logp.dtype == np.float64
        refs = check(got, score, c["x32"], c["init"], c["lengths"], c["labels"], c["paths"], c["out_len"], c["n_valid"], band)
        by_band[band] = refs, got.logp, score
    order = sorted(b for b in by_band if b) + ([0] if 0 in by_band else [])
    for lo_b, hi_b in zip(order, order[1:]):
        if hi_b and hi_b < 2 * lo_b:
            continue  # (31 -> 32: nested all the same, but the property is stated for W and 2W or more)
        g_lo, g_hi, s_lo, s_hi = by_band[lo_b][1], by_band[hi_b][1], by_band[lo_b][2], by_band[hi_b][2]
        for (b, i) in by_band[lo_b][0]:
            Tr = c["T"] if c["lengths"] is None else int(c["lengths"][b])
            if g_lo[b, i] == g_lo[b, i] and g_hi[b, i] == g_hi[b, i]:
                assert g_lo[b, i] <= g_hi[b, i] or (math.isfinite(g_hi[b, i]) and
                                                    g_lo[b, i] - g_hi[b, i] <= 1e-12 * max(1.0, abs(g_hi[b, i]))), \
                    (c["name"], b, i, lo_b, hi_b, g_lo[b, i], g_hi[b, i])
            if s_lo[b, i] == s_lo[b, i] and s_hi[b, i] == s_hi[b, i]:
                assert s_lo[b, i] <= s_hi[b, i] + 2 * tolerance(Tr) or s_lo[b, i] == s_hi[b, i], \
                    (c["name"], b, i, lo_b, hi_b, s_lo[b, i], s_hi[b, i])
    return by_band


def greedy_posteriors(rng, B, T, S, N):
    """every (t, s) row has one entry >= 0.99 and every other entry <= 0.001; about a third of the rows emit.  float32"""
    x = rng.random((B, T, S, N)) * 0.0009  # (margins that survive the rounding to f16)
    top = np.where(rng.random((B, T, S)) < 0.35, rng.integers(1, N, (B, T, S)), 0)
    np.put_along_axis(x, top[..., None], 0.992 + 0.007 * rng.random((B, T, S, 1)), -1)
    return x.astype(np.float32)


def greedy_parity(fcd, T, dtype, device=None, S=16, N=5):
    """Aligning crf_greedy_search's own labelling returns its path as start and its qualities bit for bit: greedy's own
    product is at least 0.99^200 > 0.13, and any other alignment of its labelling takes a non-maximal entry (<= 0.001) at
    its first divergence."""
    assert T <= 200
    B = 6
    rng = np.random.default_rng(2000 + T + (dtype == "f16"))
    x = greedy_posteriors(rng, B, T, S, N)
    if dtype == "f16":
        x = x.astype(np.float16)
    x32 = x.astype(np.float32)
    srt = np.sort(x32, -1)
    assert (srt[..., -1] >= 0.99).all() and (srt[..., -2] <= 0.001).all()  # (on the array the kernels read)
    init = rng.random((B, S)).astype(np.float32)
    lengths = rng.integers(max(1, T // 2), T + 1, size=B).astype(np.int64)
    lengths[0] = T
    if device is None:
        xin, lin, iin = x, lengths, init
    else:
        import torch
        xin, lin, iin = torch.from_numpy(x).to(device), torch.from_numpy(lengths).to(device), torch.from_numpy(init).to(device)
    r = fcd.crf_greedy_search_batch_raw(xin, iin, lin, qual=True)
    rc = r.cpu()
    assert (np.asarray(rc.status) == 0).all()
    for band in (0, 4):
        got = fcd.crf_align_batch_raw(xin, iin, r.labels, r.out_len, lin, r.path if band else None, band).cpu()
        for b in range(B):
            n = int(rc.out_len[b])
            assert n > 0 or lengths[b] < 4
            assert got.start[b, 0, :n].tolist() == np.asarray(rc.path[b, :n]).astype(np.uint32).tolist(), (T, dtype, band, b)
            assert (got.count[b, 0, :n] == 1).all()
            assert got.qual[b, 0, :n].view(np.uint32).tolist() == np.asarray(rc.qual[b, :n]).view(np.uint32).tolist(), (T, dtype, band, b)
