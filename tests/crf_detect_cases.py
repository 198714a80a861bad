"""TEST INFRASTRUCTURE of tests/test_crf_detect_emu.py and tests/test_gpu_crf_detect.py: a fixed, seeded table of cases through
crf_detect_batch_raw (or fcd_crf_detect_host itself) against tests/crf_detect_reference.py.

Inputs: seeded N(0, 1) raw scores with +6 on the edges of planted paths (stays, then a motif one label a row), turned into
p and marg by the float64 statements of tests/crf_transitions_reference.py and tests/crf_marginals_reference.py and rounded to
f32 (p further to f16 / bf16 where the case says so): kernel and reference read the SAME numbers.  The tie case apart:
values from {0, 1/2, 1}, every product and sum exact in f32, a tie required and the earliest row to win.

Condition on the inputs, asserted from the reference's own numbers: the best c_u leads the runner-up by 1 + 2^-12, and count is 0
or at least 2^-100.  A c_u below 2^-140 is not compared (a cell below 2^-190 loses bits at the fixed scale 2^64, one below
2^-213 counts as 0: over at most 130 * 300 cells that is below 2^-174 in sum, 2^-34 of what is compared); its track must
stay below ln 2^-139.  end is exact.

The bound, in 2^-24, for a range of n rows and ne = nb^(m-h+1) entry states.  All terms are non-negative, so a sum's relative
error is at most its worst term's; a path into c_u crosses at most n rows, and the f32 roundings on it are
  2 n      one multiply and one add a row (both products are formed at the source, the fixed scale is exact);
  ne - 1   the adds of e_u;
  1        the second-order terms of (1 + 2^-24)^(2 n + ne), 2 n + ne <= 1284
so count (a float64 sum of such terms) is within (2 n + ne) 2^-24 of the reference RELATIVELY and logp = ln c_end within the
same ABSOLUTELY (ln(1 + x) <= x).  track adds tests/ctc_spot_cases.py's three terms for logf, the exponent times ln 2 and
the multiply-add, 3 + 2 |ln v|."""
import ctypes as C
import math
import zlib

import numpy as np

import crf_detect_reference as R
import crf_marginals_reference as MR
import crf_transitions_reference as TR

NO_HIT = 0xFFFFFFFF
bound = lambda n, ne: (2 * n + ne) * 2.0 ** -24  # noqa: E731
track_bound = lambda n, ne, ln_v: (2 * n + ne + 3 + 2 * abs(ln_v)) * 2.0 ** -24  # noqa: E731

_M = lambda L, nb: [1 + (k + k // 3) % nb for k in range(L)]  # noqa: E731
_RAGGED = dict(S=16, N=5, T=130, B=4, lengths=[130, 0, 77, 9], motifs=[_M(24, 4), [4, 3, 2, 1], [2]],
               plant=[(0, 0, 60), (0, 1, 100), (2, 0, 40), (2, 1, 10), (3, 1, 3)])
# plant: (read, motif, the row of its first label); motifs of one case share a stride
CASES = {
    **{"shape_S%d_N%d_L%d" % (S, N, L): dict(S=S, N=N, T=T, motifs=[_M(L, N - 1)], plant=[(0, 0, 2)])
       for S, N, T in ((4, 3, 7), (4, 5, 7), (16, 5, 7), (64, 5, 9), (1024, 5, 9))
       for L in sorted({1, R.history(S, N), R.history(S, N) + 1})},
    **{"rows_T%d" % T: dict(S=4, N=3, T=T, motifs=[[1, 2, 2]], plant=[(0, 0, max(T - 5, 0))]) for T in (1, 7, 65, 130)},
    "K1_L24_gather": dict(S=1024, N=5, T=40, motifs=[_M(24, 4)], plant=[(0, 0, 9)]),
    "K2_L70": dict(S=64, N=5, T=130, motifs=[_M(70, 4)], plant=[(0, 0, 31)]),
    "K8_L300": dict(S=4, N=5, T=310, motifs=[_M(300, 4)], plant=[(0, 0, 4)]),
    "overlap_121_twice": dict(S=4, N=3, T=9, motifs=[[1, 2, 1], [1, 2, 1, 2, 1]], plant=[(0, 1, 2)], bonus=4.0, about=(0, 0, 2.0)),
    "ragged_M3": _RAGGED,
    "ragged_rows_inside": dict(_RAGGED, rows=(5, 70), plant=[(0, 0, 20), (0, 1, 100), (2, 0, 40), (2, 1, 10), (3, 1, 5)]),
    "ragged_rows_negative_lo": dict(_RAGGED, rows=(-40, None), plant=[(0, 0, 95), (0, 1, 20), (2, 0, 45), (2, 1, 70), (3, 1, 3)]),
    "empty_range": dict(S=4, N=5, T=65, motifs=[[1, 2]], plant=[(0, 0, 30)], rows=(40, 12)),
    "range_shorter_than_motif": dict(S=4, N=5, T=65, motifs=[_M(24, 4)], plant=[(0, 0, 30)], rows=(30, 40)),
    "no_track": dict(S=16, N=5, T=65, motifs=[_M(24, 4)], plant=[(0, 0, 30)], track=False),
    "f16": dict(S=16, N=5, T=130, dtype="f16", motifs=[_M(24, 4)], plant=[(0, 0, 60)]),
    "bf16_gather": dict(S=1024, N=5, T=9, dtype="bf16", motifs=[_M(6, 4)], plant=[(0, 0, 1)]),
    "bad_label_and_n_valid": dict(_RAGGED, motifs=[_M(24, 4), [4, 5, 2, 1], [2]], plant=[(0, 0, 20), (2, 0, 40)], bonus=2.0, host=True),
    "nan_marg_inside_and_outside": dict(S=16, N=5, T=65, B=2, rows=(10, 50), motifs=[[1, 2, 3]], plant=[(0, 0, 20), (1, 0, 20)],
                                        nan=[(0, 30), (1, 55)]),
    **{"expected_count_S4_N%d_%s" % (N, "".join(map(str, y))): dict(prop=y, N=N) for N in (3, 5) for y in ([1, 2], [1, 1], [1, 2, 1], [2])},
    "tie_halves": dict(tie=True),
    "refusals": dict(refusals=True),
}


def build(name):
    k = CASES[name]
    S, N, T, B = k["S"], k["N"], k["T"], k.get("B", 1)
    nb, rng = N - 1, np.random.default_rng(zlib.crc32(name.encode()))
    stride = max(len(y) for y in k["motifs"])
    motifs = np.array([y + [0] * (stride - len(y)) for y in k["motifs"]], np.uint8)
    lengths = None if "lengths" not in k else np.array(k["lengths"], np.int64)
    x = rng.standard_normal((B, T, S, N)).astype(np.float32)
    for r, i, row in k["plant"]:
        s, syms = 0, [0] * row + list(k["motifs"][i])
        for t, a in enumerate((syms + [0] * T)[:T]):
            x[r, t, s, a] += k.get("bonus", 6.0)
            s = s if a == 0 else (s * nb) % S + a - 1
    p, marg = np.zeros((B, T, S, N), np.float32), np.zeros((B, T, S, N), np.float32)
    for r in range(B):
        Tr = T if lengths is None else int(lengths[r])
        if Tr:
            p[r, :Tr] = TR.transitions64(x[r, :Tr])["probs"]
            marg[r, :Tr] = MR.marginals64(x[r, :Tr])["marg"]
    for r, t in k.get("nan", []):
        marg[r, t] = np.nan
    pin, kw = p, {}
    if k.get("dtype") == "f16":
        pin = p.astype(np.float16)
        p = pin.astype(np.float32)
    elif k.get("dtype") == "bf16":
        pin, kw = (p.view(np.uint32) >> 16).astype(np.uint16), dict(input_dtype="bfloat16")
        p = (pin.astype(np.uint32) << 16).view(np.float32)
    return dict(name=name, p=p, pin=pin, kw=kw, marg=marg, motifs=motifs, lens=np.array([len(y) for y in k["motifs"]], np.uint32),
                lengths=lengths, rows=k.get("rows"), track=k.get("track", True), T=T, host=k.get("host"),
                about=k.get("about"))


def close(got, want, tol):
    return got == want or (math.isnan(got) and math.isnan(want)) or abs(got - want) <= tol


def check(got, c, n_valid=None, tie=False):
    S, N = c["p"].shape[2:]
    m = R.history(S, N)
    if c.get("about"):  # the planted labelling holds the motif that often, overlaps included
        r, i, want = c["about"]
        assert abs(float(got.count[r, i]) - want) < 0.25, (c["name"], got.count[r, i])
    for r, i in np.ndindex(got.end.shape):
        Tr = c["T"] if c["lengths"] is None else int(c["lengths"][r])
        b, e, _ = slice(*(c["rows"] or (None, None))).indices(Tr)
        where, L, n = (c["name"], r, i), int(c["lens"][i]), max(e - b, 0)
        ne = (N - 1) ** (m - min(L, m) + 1)
        ref = R.crf_detect(c["p"][r, :Tr], c["marg"][r, :Tr], c["motifs"][i, :L], b, e)
        if n_valid is not None and i >= int(n_valid[r]):
            ref = dict(logp=math.nan, count=math.nan, end=None, c=None)
        if ref["end"] is not None:  # the condition on the inputs
            best = sorted(ref["c"])[::-1]
            assert ref["count"] >= 2.0 ** -100, where
            if tie:
                assert best[0] == best[1] and ref["end"] == b + ref["c"].index(best[0]), where + ("no tie in the tie case",)
            else:
                assert len(best) == 1 or best[0] >= best[1] * (1 + 2.0 ** -12), where + tuple(best[:2])
        count, trk = float(got.count[r, i]), None if got.track is None else got.track[r, i]
        assert close(count, ref["count"], bound(n, ne) * ref["count"] if ref["end"] is not None else 0.0), where + (count, ref["count"])
        assert got.logp is None or close(float(got.logp[r, i]), ref["logp"], bound(n, ne)), where + (got.logp[r, i], ref["logp"])
        assert got.end[r, i] == (NO_HIT if ref["end"] is None else ref["end"]), where + (got.end[r, i], ref["end"])
        if trk is not None and ref["c"] is not None:
            assert np.isneginf(trk[:b]).all() and np.isneginf(trk[b + n:]).all(), where  # (outside the range: untouched)
            for t, v in enumerate(ref["c"], b):
                if v and v < 2.0 ** -140:
                    assert trk[t] <= math.log(2.0 ** -139), where + (t, trk[t], v)
                else:
                    want = math.log(v) if v else -math.inf
                    assert close(float(trk[t]), want, track_bound(t - b + 1, ne, want) if v else 0.0), where + (t, trk[t], want)


def _raw_call(c, band=0, every=False, marg=True, N=None):
    """fcd_crf_detect_host itself -> (status, message, DetectResult-like arrays, n_valid)"""
    import fast_ctc_decode_amd as fcd
    from fast_ctc_decode_amd import _native as nat
    (B, T, S, N0), (M, stride) = c["p"].shape, c["motifs"].shape
    labels, ylen = np.tile(c["motifs"][None], (B, 1, 1)), np.tile(c["lens"][None], (B, 1))
    opt = [c["lengths"], np.array([3, 1, 0, 2], np.uint32), np.zeros((B, M)), np.full((B, M, T), -np.inf, np.float32),
           np.zeros(B, np.uint32), np.full(B, 70, np.uint32)] if every else [None] * 6
    lengths, n_valid, logp, track, rb, re = [a.ctypes.data if every else None for a in opt]
    count, end = np.zeros((B, M)), np.zeros((B, M), np.uint32)
    b_ = nat.Batch(c["p"].ctypes.data, B, T, S, N or N0, T * S * N0, S * N0, N0, 1, lengths)
    y_ = nat.Labellings(labels.ctypes.data, ylen.ctypes.data, n_valid, None, M, stride)
    out = nat.CrfDetect(count.ctypes.data, end.ctypes.data, logp, track, T, rb, re, c["marg"].ctypes.data if marg else None,
                        T * S * N0, S * N0, N0)
    h = nat.default_handle()
    rc = h.lib.fcd_crf_detect_host(h.ptr, C.byref(b_), C.byref(y_), band, C.byref(out))
    return rc, (h.lib.fcd_last_error(h.ptr) or b"").decode(), fcd.DetectResult(count, end, opt[2], opt[3]), opt[1]


def run_refusals():
    """each refused with its status and message before anything is written"""
    from fast_ctc_decode_amd import _native as nat
    c = build("shape_S4_N5_L2")
    wide = dict(c, motifs=np.ones((1, 513), np.uint8))  # m = 1: L - h + 1 = 513 cells
    for kw, status, text, case in ((dict(band=1), nat.E_INVALID, "band must be 0", c), (dict(marg=False), nat.E_INVALID, "null marg", c),
                                   (dict(N=4), nat.E_UNSUPPORTED, "power of N - 1", c), (dict(), nat.E_UNSUPPORTED, "512", wide)):
        rc, msg, got, _ = _raw_call(case, **kw)
        assert rc == status and text in msg and not got.end.any() and not got.count.any(), (kw, rc, msg)


def run_tie(fcd, device):
    """S = 4, N = 3 (m = 2): motif [1] ties at rows 0, 2, 5 (c = 1/2), motif [1, 2, 1] at rows 1 and 2 (c = 1/4)"""
    p, marg = np.zeros((1, 6, 4, 3), np.float32), np.zeros((1, 6, 4, 3), np.float32)
    marg[0, [0, 2, 5], 3, 1] = 0.5  # motif [1]: e_u over all four states
    marg[0, 0, 0, 2] = 0.5          # motif [1, 2, 1]: e_0 = 1/2 into cell 2, whose state is 1
    p[0, 1, 1] = [0.5, 0.5, 0]      # c_1 = 1/2 * 1/2, a_1 = 1/4
    p[0, 2, 1] = [0, 1, 0]          # c_2 = 1/4 * 1
    c = dict(name="tie_halves", p=p, marg=marg, motifs=np.array([[1, 0, 0], [1, 2, 1]], np.uint8), lens=np.array([1, 3], np.uint32),
             lengths=None, rows=None, T=6)
    to = (lambda a: a) if device is None else (lambda a: __import__("torch").from_numpy(a).to(device))
    got = fcd.crf_detect_batch_raw(to(p), to(marg), c["motifs"], c["lens"], track=True).cpu()
    assert list(got.end[0]) == [0, 1] and list(got.count[0]) == [1.5, 0.5], (got.end, got.count)
    check(got, c, tie=True)


def run_property(fcd, y, N, device):
    """the reference's count IS the brute-force expected count (1e-12); the kernel's (and crf_detect's) within the bound"""
    x = np.random.default_rng(7 + N).standard_normal((6, 4, N)).astype(np.float32)
    p, marg = TR.transitions64(x)["probs"], MR.marginals64(x)["marg"]
    ref, want = R.crf_detect(p, marg, y), R.expected_count(x, y)
    assert abs(ref["count"] - want) <= 1e-12 and want > 0.01, (ref["count"], want)
    to = (lambda a: a) if device is None else (lambda a: __import__("torch").from_numpy(a).to(device))
    c = dict(name="expected_count", p=p.astype(np.float32)[None], marg=marg.astype(np.float32)[None], motifs=np.array([y], np.uint8),
             lens=np.array([len(y)], np.uint32), lengths=None, rows=None, T=6)
    check(fcd.crf_detect_batch_raw(to(c["p"]), to(c["marg"]), c["motifs"], c["lens"], track=True).cpu(), c)
    if device is None:  # the one-read call from raw scores: its own p and marg, each within a few f32 roundings of these
        one = fcd.crf_detect(x, "".join("NAC"[v] if N == 3 else "NACGT"[v] for v in y), "NAC" if N == 3 else "NACGT")
        assert abs(one[0] - want) <= 1e-4 * want and one[1] is not None, (one, want)


def run_case(fcd, name, device=None):
    k = CASES[name]
    if "prop" in k:
        return run_property(fcd, k["prop"], k["N"], device)
    if k.get("tie"):
        return run_tie(fcd, device)
    if k.get("refusals"):
        return run_refusals()
    c = build(name)
    if c["host"] and device is None:  # fcd_crf_detect_host itself, every nullable pointer set (n_valid = 3, 1, 0, 2; rows 0 .. 70)
        rc, msg, got, n_valid = _raw_call(c, every=True)
        assert rc == 0, msg
        return check(got, dict(c, rows=(0, 70)), n_valid)
    pin, marg, lengths = c["pin"], c["marg"], c["lengths"]
    if device is not None:
        import torch
        dev = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
        pin, marg = (dev(pin.view(np.int16)).view(torch.bfloat16) if c["kw"] else dev(pin)), dev(marg)
        lengths = None if lengths is None else dev(lengths)
    kw = c["kw"] if device is None else {}
    check(fcd.crf_detect_batch_raw(pin, marg, c["motifs"], c["lens"], lengths, c["rows"], track=c["track"], **kw).cpu(), c)
