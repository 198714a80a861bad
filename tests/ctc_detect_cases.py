"""TEST INFRASTRUCTURE of tests/test_ctc_detect_emu.py and tests/test_gpu_ctc_detect.py: a fixed, seeded table of cases
through ctc_detect_batch_raw (or fcd_ctc_detect_host itself) against tests/ctc_detect_reference.py.  Posteriors k / 256 from
tests/ctc_spot_cases.py's generator run on this table (background 16 .. 48, the motif planted at 230 .. 235, one row a
label; the rows sum to 1 in the property test, here the arithmetic is the definition).  Condition, asserted from the reference's own numbers (the tie
case apart: posteriors from {0, 1/2, 1}, every product and sum exact in f32, a tie required): the best c_t leads the
runner-up by 1 + 2^-12, and count is 0 or at least 2^-150.  A c_t below 2^-200 is not compared (the kernels may drop what
lies below 2^-245; all they drop is below 2^-229 in sum: 2^16 cells); its track must stay below ln 2^-199.  end is exact.
The bound, in 2^-24, for a range of n rows.  All terms are non-negative, so a sum's relative error is at most its worst
term's; a path into c_t crosses at most n rows, and the f32 roundings on it are
  3 n     two adds and the posterior multiply a row;
  1 + 2   1 - p of the entry weight; 1 - p of the exit weight and the exit multiply;
  1       the second-order terms of (1 + 2^-24)^(3 n + 3), n <= 262
so count (a float64 sum of such terms) is within (3 n + 4) 2^-24 of the reference RELATIVELY and logp = ln c_end within the
same ABSOLUTELY (ln(1 + x) <= x).  track adds tests/ctc_spot_cases.py's three terms for logf, the exponent times ln 2
and the multiply-add, 3 + 2 |ln v|:  (3 n + 7 + 2 |ln v|) 2^-24, a = 3, b = 7, c = 2."""
import ctypes as C
import math

import numpy as np

import ctc_align_cases as AC
import ctc_detect_reference as R
import ctc_spot_cases as SP

bound = lambda n: (3 * n + 4) * 2.0 ** -24  # noqa: E731
track_bound = lambda n, ln_v: (3 * n + 7 + 2 * abs(ln_v)) * 2.0 ** -24  # noqa: E731

# (as tests/ctc_spot_cases.py) host: fcd_ctc_detect_host, the nullable pointers all null or all set (and n_valid = 3, 1, 0, 2)
_M24 = [1 + (7 * k * k + k) % 4 for k in range(24)]
_M24 = [v if k == 0 or v != _M24[k - 1] else 1 + v % 4 for k, v in enumerate(_M24)]
_M260 = [1 + (k + k // 4) % 4 for k in range(260)]
_HALVES = [[.5, .5, 0], [1, 0, 0], [.5, .5, 0], [1, 0, 0], [0, 0, 1], [.5, .5, 0]]  # motif [1]: c = 1/2, 0, 1/2, 0, 0, 1/2
_RAGGED = dict(T=130, N=5, stride=24, B=4, lengths=[130, 0, 77, 9], rows=(0, 70), motifs=[_M24[:8], [4, 3, 2, 1], _M24[:8]],
               plant=[(0, 0, 60, 230), (0, 1, 90, 230), (2, 0, 66, 230), (2, 1, 10, 230), (3, 1, 3, 230)])
CASES = {
    "L1_T1": dict(T=1, N=5, stride=4, motifs=[[3]], plant=[(0, 0, 0, 230)]),
    "L2_repeat_T7": dict(T=7, N=5, stride=4, motifs=[[2, 2]], plant=[(0, 0, 2, 230)]),
    "L2_repeat_T7_nocollapse": dict(T=7, N=5, stride=4, motifs=[[2, 2]], plant=[(0, 0, 2, 230)], collapse=False),
    "overlap_121": dict(T=9, N=5, stride=8, motifs=[[1, 2, 1], [1, 2, 1, 2, 1]], plant=[(0, 1, 2, 230)]),
    "first_possible_row_K2": dict(T=65, N=5, stride=24, motifs=[_M24], plant=[(0, 0, 0, 230)]),
    "last_row_K4": dict(T=65, N=5, stride=65, motifs=[_M260[:60]], plant=[(0, 0, 5, 230)]),
    "across_chunk_and_tile_K6": dict(T=130, N=5, stride=130, motifs=[_M260[:125]], plant=[(0, 0, 3, 230)]),
    "long_motif_K8": dict(T=200, N=5, stride=200, motifs=[_M260[:190]], plant=[(0, 0, 6, 230)]),
    "lds_260_labels": dict(T=262, N=5, stride=260, motifs=[_M260], plant=[(0, 0, 1, 230)]),
    "absent_zero_column": dict(T=65, N=5, stride=8, motifs=[[1, 4, 2]], plant=[], zero=4),
    "ragged_rows_head": _RAGGED,
    "ragged_rows_tail": dict(_RAGGED, rows=(-40, None), plant=[(0, 0, 121, 230), (0, 1, 20, 230), (2, 0, 40, 230), (2, 1, 70, 230), (3, 1, 3, 230)]),
    "host_abi_all_null": dict(_RAGGED, host=False),
    "host_abi_all_set": dict(_RAGGED, host=True),
    "empty_range": dict(T=65, N=5, stride=8, motifs=[[1, 2]], plant=[(0, 0, 30, 230)], rows=(40, 12)),
    "f16": dict(T=130, N=5, stride=24, dtype="f16", motifs=[_M24], plant=[(0, 0, 60, 230)]),
    "bf16": dict(T=130, N=5, stride=24, dtype="bf16", motifs=[_M24], plant=[(0, 0, 60, 230)]),
    "time_major": dict(T=130, N=5, stride=24, B=3, time_major=True, motifs=[_M24], plant=[(0, 0, 5, 230), (1, 0, 100, 230), (2, 0, 60, 230)]),
    "nan_inside_and_outside": dict(T=65, N=5, stride=8, B=2, rows=(10, 50), motifs=[[1, 2, 3]], plant=[(0, 0, 20, 230), (1, 0, 20, 230)],
                                   nan=[(0, 30), (1, 55)]),
    **{"expected_count_%s%s" % ("".join(map(str, y)), "" if cr else "_nocollapse"): dict(prop=y, collapse=cr)
       for y in ([1, 2], [1, 1], [1, 2, 1]) for cr in (True, False)},
    "tie_halves": dict(T=6, N=3, stride=4, motifs=[[1], [2, 1]], plant=[], matrix=_HALVES),
}


def build(name):
    saved, SP.CASES = SP.CASES, CASES  # (the generator reads its module's table: this one, for the length of the call)
    try:
        c = SP.build(name)
    finally:
        SP.CASES = saved
    if "matrix" in CASES[name]:
        c["x32"] = c["xin"] = np.array([CASES[name]["matrix"]], np.float32)
    c["host"] = CASES[name].get("host")
    if c["host"] is False:
        c["lengths"] = c["rows"] = None
    return c


def close(got, want, tol):
    return got == want or (math.isnan(got) and math.isnan(want)) or abs(got - want) <= tol


def check(got, c, n_valid=None):
    for r, i in np.ndindex(got.end.shape):
        Tr = c["T"] if c["lengths"] is None else int(c["lengths"][r])
        b, e, _ = slice(*(c["rows"] or (None, None))).indices(Tr)
        where, L, n = (c["name"], r, i), int(c["lens"][i]), max(e - b, 0)
        ref = R.ctc_detect(c["x32"][r, :Tr], c["motifs"][i, :L], c["collapse"], b, e)
        if n_valid is not None and i >= int(n_valid[r]):
            ref = dict(logp=math.nan, count=math.nan, end=None, c=None)
        if ref["end"] is not None:  # the condition on the inputs
            best = sorted(ref["c"])[::-1]
            assert ref["count"] >= 2.0 ** -150, where
            if "matrix" in CASES[c["name"]] and i == 0:
                assert best[0] == best[1] and ref["end"] == b + ref["c"].index(best[0]), where + ("no tie in the tie case",)
            else:
                assert len(best) == 1 or best[0] >= best[1] * (1 + 2.0 ** -12), where + tuple(best[:2])
        count, trk = float(got.count[r, i]), None if got.track is None else got.track[r, i]
        assert close(count, ref["count"], bound(n) * ref["count"] if ref["end"] is not None else 0.0), where + (count, ref["count"])
        assert got.logp is None or close(float(got.logp[r, i]), ref["logp"], bound(n)), where + (got.logp[r, i], ref["logp"])
        assert got.end[r, i] == (SP.NO_HIT if ref["end"] is None else ref["end"]), where + (got.end[r, i], ref["end"])
        if trk is not None and ref["c"] is not None:
            assert np.isneginf(trk[:b]).all() and np.isneginf(trk[b + n:]).all(), where  # (outside the range: untouched)
            for t, v in enumerate(ref["c"], b):
                if v and v < 2.0 ** -200:
                    assert trk[t] <= math.log(2.0 ** -199), where + (t, trk[t], v)
                else:
                    want = math.log(v) if v else -math.inf
                    assert close(float(trk[t]), want, track_bound(t - b + 1, want) if v else 0.0), where + (t, trk[t], want)


def call_host(fcd, c):  # fcd_ctc_detect_host itself: band 1 is refused before anything is written, band 0 runs and is checked
    from fast_ctc_decode_amd import _native as nat
    (B, T, N), (M, stride), every = c["x32"].shape, c["motifs"].shape, c["host"]
    labels, ylen = np.tile(c["motifs"][None], (B, 1, 1)), np.tile(c["lens"][None], (B, 1))
    opt = [c["lengths"], np.array([3, 1, 0, 2], np.uint32), np.zeros((B, M)), np.full((B, M, T), -np.inf, np.float32),
           np.zeros(B, np.uint32), np.minimum(70, c["lengths"]).astype(np.uint32)] if every else [None] * 6
    lengths, n_valid, logp, track, rb, re = [a.ctypes.data if every else None for a in opt]
    count, end = np.zeros((B, M)), np.zeros((B, M), np.uint32)
    b_ = nat.Batch(c["x32"].ctypes.data, B, T, 1, N, T * N, N, 0, 1, lengths)
    y_ = nat.Labellings(labels.ctypes.data, ylen.ctypes.data, n_valid, None, M, stride)
    out, h = nat.Detect(count.ctypes.data, end.ctypes.data, logp, track, T, rb, re), nat.default_handle()
    assert h.lib.fcd_ctc_detect_host(h.ptr, C.byref(b_), C.byref(y_), 1, 1, C.byref(out)) == nat.E_INVALID and not end.any()
    assert h.lib.fcd_ctc_detect_host(h.ptr, C.byref(b_), C.byref(y_), 1, 0, C.byref(out)) == nat.OK, h.lib.fcd_last_error(h.ptr)
    check(fcd.DetectResult(count, end, opt[2], opt[3]), c, opt[1])


def run_case(fcd, name, device=None):
    if "prop" in CASES[name]:
        return run_property(fcd, CASES[name]["prop"], CASES[name].get("collapse", True), device)
    c = build(name)
    if c["host"] is not None and device is None:
        return call_host(fcd, c)
    xin, conv, kw = AC._device_inputs(c, device)  # (f16 / bf16 / time-major, on the device too)
    check(fcd.ctc_detect_batch_raw(xin, c["motifs"], c["lens"], c["collapse"], conv(c["lengths"]), c["rows"], track=True, **kw).cpu(), c)


def run_property(fcd, y, collapse, device=None):
    """normalised rows: the reference's count IS the brute-force expected count (1e-12); the kernel's (and ctc_detect's) within the bound"""
    x = np.array([[10, 40, 14], [30, 10, 24], [8, 44, 12], [20, 12, 32], [12, 38, 14], [24, 20, 20]], np.float32) / 64
    ref, want = R.ctc_detect(x, y, collapse), R.expected_count(x, y, collapse)
    assert abs(ref["count"] - want) <= 1e-12 and want > 0.01, (ref["count"], want)
    xin = x[None] if device is None else __import__("torch").from_numpy(x[None]).to(device)
    got = fcd.ctc_detect_batch_raw(xin, np.array([y + [0] * (4 - len(y))], np.uint8), np.array([len(y)], np.uint32), collapse).cpu()
    assert close(float(got.count[0, 0]), ref["count"], bound(6) * ref["count"]), (got.count, ref["count"])
    if collapse and device is None:
        one = fcd.ctc_detect(x, "".join("NAC"[v] for v in y), "NAC", rows=(0, 6))
        assert one == (float(got.count[0, 0]), ref["end"], float(got.logp[0, 0])) and fcd.ctc_detect(x, "", "NAC")[:2] == (0.0, None)
