"""TEST INFRASTRUCTURE of tests/test_ctc_spot_emu.py and tests/test_gpu_ctc_spot.py: a fixed, seeded table of motif-spotting
cases through ctc_spot_batch_raw against tests/ctc_spot_reference.py.  Posteriors k / 256 (exact in f16 / bf16), background
16 .. 48, the motif planted at 225 .. 240, one row a label.  Condition, asserted from the reference's own numbers (tie cases
apart: posteriors k / 4, every product exact, a tie required): every decision of the best hit holds by 1 + 2^-12 (a path's
f32 roundings, 260 rows at most, stay below 1 + 2^-15) and no cell lies below 2^-200 (the kernels drop below 2^-245).  Under
it start, count, end, qual are compared exactly, logp with ctc_align_cases.logp_same, track with track_bound, in 2^-24:
  n          a path into the cell has at most n = t - b + 1 factors, each product rounded once to f32 (ln(1 + x) < x);
  2          logf of the mantissa in [0.5, 1): within 2 ulp of a result in (-0.70, 0], whose ulp is 2^-24 at most;
  |E| / 2    the exponent E (|E| <= |ln v| / ln 2 + 1) times ln 2 as an f32 constant, off by half an ulp of 2^-24;
  |ln v|     the one rounding of the multiply-add; in all n + 2.5 + |ln v| (1 + 1 / (2 ln 2)) <= n + 3 + 2 |ln v|."""
import math

import numpy as np

import ctc_align_cases as AC
import ctc_spot_reference as R

NO_HIT = 0xFFFFFFFF


def track_bound(n, ln_v):
    return (n + 3 + 2 * abs(ln_v)) * 2.0 ** -24


# plant = [(read, motif, row, k of the planted posteriors)]; zero: a label whose column is 0; nan = [(read, row)]
_M24 = [1 + (7 * k * k + k) % 4 for k in range(24)]
_M24 = [v if k == 0 or v != _M24[k - 1] else 1 + v % 4 for k, v in enumerate(_M24)]
_M40 = [1 + (k + k // 4) % 4 for k in range(40)]
CASES = {
    "L1_T1": dict(T=1, N=5, stride=4, motifs=[[3]], plant=[(0, 0, 0, 230)]),
    "L2_repeat_T7": dict(T=7, N=5, stride=4, motifs=[[2, 2]], plant=[(0, 0, 2, 230)]),
    "L2_repeat_T7_nocollapse": dict(T=7, N=5, stride=4, motifs=[[2, 2]], plant=[(0, 0, 2, 230)], collapse=False),
    "hit_at_row0_K2": dict(T=65, N=5, stride=24, motifs=[_M24], plant=[(0, 0, 0, 230)]),
    "hit_at_last_row_K4": dict(T=65, N=5, stride=65, motifs=[_M24], plant=[(0, 0, 41, 230)]),
    "across_chunk_K6": dict(T=130, N=5, stride=130, motifs=[_M24], plant=[(0, 0, 50, 230)]),
    "two_copies_K8": dict(T=200, N=5, stride=200, motifs=[_M24], plant=[(0, 0, 20, 215), (0, 0, 120, 235)]),
    "lds_two_wavefronts": dict(T=260, N=5, stride=256, motifs=[_M40], plant=[(0, 0, 100, 232)]),
    "absent_zero_column": dict(T=65, N=5, stride=8, motifs=[[1, 4, 2]], plant=[], zero=4),
    "ragged_rows_head": dict(T=130, N=5, stride=24, B=4, lengths=[130, 0, 77, 9], rows=(0, 70), motifs=[_M24[:8], [4, 3, 2, 1]],
                             plant=[(0, 0, 60, 230), (0, 1, 90, 238), (2, 0, 66, 230), (2, 1, 10, 230), (3, 1, 3, 230)]),
    "ragged_rows_tail": dict(T=130, N=5, stride=24, B=4, lengths=[130, 0, 77, 9], rows=(-40, None), motifs=[_M24[:8], [4, 3, 2, 1]],
                             plant=[(0, 0, 121, 230), (0, 1, 20, 238), (2, 0, 30, 238), (2, 1, 70, 230), (3, 1, 3, 230)]),
    "empty_range": dict(T=65, N=5, stride=8, motifs=[[1, 2]], plant=[(0, 0, 30, 230)], rows=(40, 12)),
    "f16": dict(T=130, N=5, stride=24, dtype="f16", motifs=[_M24], plant=[(0, 0, 60, 230)]),
    "bf16": dict(T=130, N=5, stride=24, dtype="bf16", motifs=[_M24], plant=[(0, 0, 60, 230)]),
    "time_major": dict(T=130, N=5, stride=24, B=3, time_major=True, motifs=[_M24], plant=[(0, 0, 5, 230), (1, 0, 100, 230), (2, 0, 60, 230)]),
    "nan_inside_and_outside": dict(T=65, N=5, stride=8, B=2, rows=(10, 50), motifs=[[1, 2, 3]], plant=[(0, 0, 20, 230), (1, 0, 20, 230)],
                                   nan=[(0, 30), (1, 55)]),
    "ties_quarters": dict(T=11, N=3, stride=4, motifs=[[1, 1, 2], [2, 1]], plant=[], quarters=True),
    "ties_quarters_nocollapse": dict(T=11, N=3, stride=4, motifs=[[1, 1, 2], [2, 1]], plant=[], quarters=True, collapse=False),
}


def build(name):
    c = dict(CASES[name])
    rng = np.random.default_rng(c.get("seed", 20260 + sorted(CASES).index(name)))
    shape, T, collapse = (c.get("B", 1), c["T"], c["N"]), c["T"], c.get("collapse", True)
    x = rng.choice([0.25, 0.5, 1.0], size=shape, p=[0.2, 0.5, 0.3]) if c.get("quarters") else rng.integers(16, 49, size=shape) / 256.0
    for read, mi, row, k in c["plant"]:
        y, t = c["motifs"][mi], row
        for j, lab in enumerate(y):
            if j and collapse and lab == y[j - 1]:
                x[read, t, 0] = (k + 5) / 256.0
                t += 1
            x[read, t, lab] = (k + int(rng.integers(0, 6))) / 256.0
            t += 1
    if "zero" in c:
        x[:, :, c["zero"]] = 0.0
    x32 = x.astype(np.float32)
    for read, row in c.get("nan", []):
        x32[read, row, 0] = np.nan
    motifs, lens = np.zeros((len(c["motifs"]), c["stride"]), np.uint8), np.array([len(y) for y in c["motifs"]], np.uint32)
    for i, y in enumerate(c["motifs"]):
        motifs[i, :len(y)] = y
    dtype = c.get("dtype", "f32")
    xin = {"f32": x32, "f16": x32.astype(np.float16), "bf16": (x32.view(np.uint32) >> 16).astype(np.uint16)}[dtype]
    if c.get("time_major"):
        xin = np.ascontiguousarray(np.moveaxis(xin, 0, 1)).transpose(1, 0, 2)  # (B, T, N) view of (T, B, N) memory
    lengths = None if "lengths" not in c else np.asarray(c["lengths"], np.int64)
    return dict(name=name, x32=x32, xin=xin, dtype=dtype, motifs=motifs, lens=lens, lengths=lengths, rows=c.get("rows"),
                collapse=collapse, exact_ties=bool(c.get("quarters")), T=T)


def check(got, c, n_valid=None):
    tied = False
    for r, i in np.ndindex(got.end.shape):
        Tr = c["T"] if c["lengths"] is None else int(c["lengths"][r])
        b, e, _ = slice(*(c["rows"] or (None, None))).indices(Tr)
        where, n = (c["name"], r, i), int(c["lens"][i])
        ref = R.ctc_spot(c["x32"][r, :Tr], c["motifs"][i, :n], c["collapse"], b, e)
        if n_valid is not None and i >= int(n_valid[r]):
            ref = dict(ref, logp=math.nan, end=None, track=None)
        elif not c["exact_ties"]:  # the condition on the inputs
            assert ref["margin"] >= 1 + 2.0 ** -12 and ref["floor"] >= 2.0 ** -200, where + (ref["margin"], ref["floor"])
        tied |= ref["tied"]
        assert got.logp is None or AC.logp_same(got.logp[r, i], ref["logp"]), where + (ref["logp"],)
        if got.track is not None and ref["track"] is not None:
            trk = got.track[r, i]
            assert np.isneginf(trk[:b]).all() and np.isneginf(trk[max(e, b):]).all(), where  # (outside the range: untouched)
            for t, want in enumerate(ref["track"], b):
                assert trk[t] == want or abs(trk[t] - want) <= track_bound(t - b + 1, want), where + (t, trk[t], want)
        if ref["end"] is None:
            assert got.end[r, i] == NO_HIT and (got.spans.count[r, i, :n] == 0).all(), where
            continue
        assert got.end[r, i] == ref["end"] and got.start[r, i] == ref["start"][0], where + (got.end[r, i], ref["end"])
        assert got.spans.start[r, i, :n].tolist() == ref["start"] and got.spans.count[r, i, :n].tolist() == ref["count"], where
        assert got.spans.qual is None or got.spans.qual[r, i, :n].tobytes() == np.asarray(ref["qual"], np.float32).tobytes(), where
    assert tied or not c["exact_ties"], (c["name"], "no tie in the tie case")


def run_case(fcd, name, device=None):
    c = build(name)
    xin, conv, kw = AC._device_inputs(c, device)  # (f16 / bf16 / time-major, on the device too)
    check(fcd.ctc_spot_batch_raw(xin, c["motifs"], c["lens"], c["collapse"], conv(c["lengths"]), c["rows"], track=True, **kw).cpu(), c)


def host_abi(fcd, every_pointer):
    """fcd_ctc_spot_host on "ragged_rows_head" with M = 3 motifs (its two and the first again): the nullable pointers all null or all set"""
    import ctypes as C
    from fast_ctc_decode_amd import _native as nat
    from fast_ctc_decode_amd.api import AlignResult, SpotResult
    c = build("ragged_rows_head")
    (B, T, N), x = c["x32"].shape, c["x32"]
    c["motifs"], c["lens"] = np.concatenate([c["motifs"], c["motifs"][:1]]), np.concatenate([c["lens"], c["lens"][:1]])
    M, stride = c["motifs"].shape
    labels, ylen = np.tile(c["motifs"][None], (B, 1, 1)), np.tile(c["lens"][None], (B, 1))
    opt = [c["lengths"], np.array([3, 1, 0, 2], np.uint32), np.zeros((B, M, stride), np.float32), np.zeros((B, M)),
           np.full((B, M, T), -np.inf, np.float32), np.zeros(B, np.uint32), np.minimum(70, c["lengths"]).astype(np.uint32)]
    lengths, n_valid, qual, logp, track, rb, re = ptr = [a.ctypes.data if every_pointer else None for a in opt]
    if not every_pointer:
        c["lengths"], c["rows"], opt = None, None, [None] * 7
    start, count, end = np.zeros((B, M, stride), np.uint32), np.zeros((B, M, stride), np.uint32), np.zeros((B, M), np.uint32)
    b_ = nat.Batch(x.ctypes.data, B, T, 1, N, T * N, N, 0, 1, lengths)
    y_ = nat.Labellings(labels.ctypes.data, ylen.ctypes.data, n_valid, None, M, stride)
    out = nat.Spot(start.ctypes.data, count.ctypes.data, qual, logp, end.ctypes.data, track, T, rb, re)
    h = nat.default_handle()
    assert h.lib.fcd_ctc_spot_host(h.ptr, C.byref(b_), C.byref(y_), 1, 1, C.byref(out)) == nat.E_INVALID and not end.any()
    assert h.lib.fcd_ctc_spot_host(h.ptr, C.byref(b_), C.byref(y_), 1, 0, C.byref(out)) == nat.OK, h.lib.fcd_last_error(h.ptr)
    check(SpotResult(AlignResult(start, count, opt[2], opt[3]), end, opt[4]), c, opt[1])
