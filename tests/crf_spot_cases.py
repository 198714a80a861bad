"""TEST INFRASTRUCTURE of tests/test_crf_spot_emu.py and tests/test_gpu_crf_spot.py: a fixed, seeded table of cases through
crf_spot_batch_raw (or fcd_crf_spot_host itself) against tests/crf_spot_reference.py.  Inputs are built by
tests/crf_detect_cases.py's build (seeded scores, planted paths, p and marg from the float64 references rounded to f32): a
case of the same name reads the same numbers as the detect case.

Condition on the inputs, asserted from the reference's own numbers: margin >= 1 + 2^-12 (the best end row over every other,
every winner over its loser on the best path: a path's f32 roundings, 310 rows at most, stay below 1 + 2^-15) and
v_hit >= 2^-100.  Under it end, first and the spans are compared exactly.  A v_u below 2^-140 is held only to staying below
ln 2^-139 (a cell below 2^-190 loses bits at the fixed scale 2^64).

The bound, in 2^-24, for a range of n rows and ne = nb^(m-h+1) entry states: a path into v_u crosses at most n rows with one
f32 product each (the scale and the max are exact), e_u adds ne - 1 roundings, second order stays below one unit: logp is
within (n + ne) 2^-24 of the reference, absolutely.  track adds tests/ctc_spot_cases.py's three terms, 3 + 2 |ln v|."""
import ctypes as C
import math
from unittest import mock

import numpy as np

import crf_detect_cases as DC
import crf_spot_reference as R
import crf_marginals_reference as MR
import crf_transitions_reference as TR

NO_HIT = DC.NO_HIT
bound = lambda n, ne: (n + ne) * 2.0 ** -24  # noqa: E731
track_bound = lambda n, ne, ln_v: (n + ne + 3 + 2 * abs(ln_v)) * 2.0 ** -24  # noqa: E731

_M, _RAGGED = DC._M, DC._RAGGED
CASES = {
    **{k: v for k, v in DC.CASES.items() if k.startswith(("shape_", "rows_T", "K", "ragged_", "empty_", "range_", "f16", "bf16_", "bad_label", "nan_marg"))},
    "no_track": dict(DC.CASES["no_track"]),
    "no_spans_no_workspace": dict(_RAGGED, spans=False),
    "device_switch_spans": dict(S=16, N=5, T=65, motifs=[_M(24, 4)], plant=[(0, 0, 30)]),
    **{"best_path_S4_N%d_%s" % (N, "".join(map(str, y))): dict(prop=y, N=N) for N in (3, 5) for y in ([1, 2], [1, 1], [1, 2, 1], [2])},
    "tie_halves": dict(tie=True),
    "refusals": dict(refusals=True),
    "detect_is_above_and_rows_ordered": dict(cross=True),
}


def build(name):
    with mock.patch.dict(DC.CASES, {name: CASES[name]}):  # (DC.build reads its own table: the same builder, this table's rows)
        return dict(DC.build(name), spans=CASES[name].get("spans", True))


def check(got, c, n_valid=None, tie=False):
    S, N = c["p"].shape[2:]
    m = R.history(S, N)
    for r, i in np.ndindex(got.end.shape):
        Tr = c["T"] if c["lengths"] is None else int(c["lengths"][r])
        b, e, _ = slice(*(c["rows"] or (None, None))).indices(Tr)
        where, L, n = (c["name"], r, i), int(c["lens"][i]), max(e - b, 0)
        h = min(L, m)
        ne = (N - 1) ** (m - h + 1)
        ref = R.crf_spot(c["p"][r, :Tr], c["marg"][r, :Tr], c["motifs"][i, :L], b, e)
        if n_valid is not None and i >= int(n_valid[r]):
            ref = dict(logp=math.nan, end=None, v=None)
        if ref["end"] is not None and not tie:  # the condition on the inputs
            assert ref["margin"] >= 1 + 2.0 ** -12 and math.exp(ref["logp"]) >= 2.0 ** -100, where + (ref["margin"], ref["logp"])
        assert got.logp is None or DC.close(float(got.logp[r, i]), ref["logp"], bound(n, ne)), where + (got.logp[r, i], ref["logp"])
        if got.track is not None and ref["v"] is not None:
            trk = got.track[r, i]
            assert np.isneginf(trk[:b]).all() and np.isneginf(trk[b + n:]).all(), where  # (outside the range: untouched)
            for t, v in enumerate(ref["v"], b):
                if v and v < 2.0 ** -140:
                    assert trk[t] <= math.log(2.0 ** -139), where + (t, trk[t], v)
                else:
                    want = math.log(v) if v else -math.inf
                    assert DC.close(float(trk[t]), want, track_bound(t - b + 1, ne, want) if v else 0.0), where + (t, trk[t], want)
        sp = got.spans
        if ref["end"] is None:
            assert got.end[r, i] == NO_HIT and got.start[r, i] == NO_HIT and (sp is None or (sp.count[r, i, :L] == 0).all()), where
            continue
        assert (got.end[r, i], got.start[r, i]) == (ref["end"], ref["first"]), where + (got.end[r, i], got.start[r, i], ref["end"], ref["first"])
        if sp is None:
            continue
        assert sp.start[r, i, h - 1:L].tolist() == ref["start"] and (sp.count[r, i, h - 1:L] == 1).all(), where + (sp.start[r, i, :L], ref["start"])
        assert (sp.start[r, i, :h - 1] == NO_HIT).all() and not sp.count[r, i, :h - 1].any() and not sp.qual[r, i, :h - 1].any(), where
        qual = [ref["e_first"]] + [c["p"][r, ref["start"][k - h + 1], ref["sigma"][k], c["motifs"][i, k]] if ref["sigma"][k] < S else 0.0
                                   for k in range(h, L)]
        assert sp.qual[r, i, h - 1:L].tobytes() == np.asarray(qual, np.float32).tobytes(), where


def _raw_call(c, band=0, every=False, marg=True, N=None, first=True, count=True):
    """fcd_crf_spot_host itself -> (status, message, SpotResult, n_valid)"""
    import fast_ctc_decode_amd as fcd
    from fast_ctc_decode_amd import _native as nat
    (B, T, S, N0), (M, stride) = c["p"].shape, c["motifs"].shape
    labels, ylen = np.tile(c["motifs"][None], (B, 1, 1)), np.tile(c["lens"][None], (B, 1))
    opt = [c["lengths"], np.array([3, 1, 0, 2], np.uint32), np.zeros((B, M)), np.full((B, M, T), -np.inf, np.float32),
           np.zeros(B, np.uint32), np.full(B, 70, np.uint32)] if every else [None] * 6
    lengths, n_valid, logp, track, rb, re = [a.ctypes.data if every else None for a in opt]
    al = fcd.AlignResult(np.zeros((B, M, stride), np.uint32), np.zeros((B, M, stride), np.uint32), np.zeros((B, M, stride), np.float32), opt[2])
    end, fst = np.zeros((B, M), np.uint32), np.zeros((B, M), np.uint32)
    b_ = nat.Batch(c["p"].ctypes.data, B, T, S, N or N0, T * S * N0, S * N0, N0, 1, lengths)
    y_ = nat.Labellings(labels.ctypes.data, ylen.ctypes.data, n_valid, None, M, stride)
    out = nat.CrfSpot(al.start.ctypes.data, al.count.ctypes.data if count else None, al.qual.ctypes.data, logp, end.ctypes.data, track, T,
                      rb, re, fst.ctypes.data if first else None, c["marg"].ctypes.data if marg else None, T * S * N0, S * N0, N0)
    h = nat.default_handle()
    rc = h.lib.fcd_crf_spot_host(h.ptr, C.byref(b_), C.byref(y_), band, C.byref(out))
    from fast_ctc_decode_amd.api import SpotResult
    return rc, (h.lib.fcd_last_error(h.ptr) or b"").decode(), SpotResult(al, end, opt[3], first=fst, logp=opt[2]), opt[1]


def run_refusals():
    """each refused with its status and message before anything is written"""
    from fast_ctc_decode_amd import _native as nat
    c = build("shape_S4_N5_L2")
    wide = dict(c, motifs=np.ones((1, 513), np.uint8))  # m = 1: L - h + 1 = 513 cells
    for kw, status, text, case in ((dict(band=1), nat.E_INVALID, "band must be 0", c), (dict(marg=False), nat.E_INVALID, "null marg", c),
                                   (dict(first=False), nat.E_INVALID, "null first", c), (dict(count=False), nat.E_INVALID, "together", c),
                                   (dict(N=4), nat.E_UNSUPPORTED, "power of N - 1", c), (dict(), nat.E_UNSUPPORTED, "512", wide)):
        rc, msg, got, _ = _raw_call(case, **kw)
        assert rc == status and "crf_spot" in msg and text in msg and not got.end.any() and not got.spans.count.any(), (kw, rc, msg)


def _to(device):
    return (lambda a: a) if device is None else (lambda a: __import__("torch").from_numpy(a).to(device))


def run_tie(fcd, device):
    """S = 4, N = 3 (m = 2), values from {0, 1/2, 1}: motif [1] ties at rows 0, 2, 5 (v = 1/2: the earliest row wins);
    motif [1, 2, 1] enters cell 2 at row 0 and again, with the same weight, at row 1 where staying ties with the entry
    (stay wins: first = 0), and v ties at rows 2 and 3 (1/4 each: end = 2)"""
    p, marg = np.zeros((1, 6, 4, 3), np.float32), np.zeros((1, 6, 4, 3), np.float32)
    marg[0, [0, 2, 5], 3, 1] = 0.5   # motif [1]: e_u over all four states
    marg[0, 0, 0, 2] = 0.5           # motif [1, 2, 1]: e_0 = 1/2 into cell 2, whose state is 1
    marg[0, 1, 0, 2] = 0.5           # e_1 = 1/2 = a_0 * p[1][1][0]: a tie, stay is kept
    p[0, 1, 1] = [1, 0, 0]           # a_1 = 1/2 (stay), v_1 = 0
    p[0, 2, 1] = [1, 0.5, 0]         # v_2 = 1/4, a_2 = 1/2
    p[0, 3, 1] = [0, 0.5, 0]         # v_3 = 1/4: the tie of end rows
    c = dict(name="tie_halves", p=p, marg=marg, motifs=np.array([[1, 0, 0], [1, 2, 1]], np.uint8), lens=np.array([1, 3], np.uint32),
             lengths=None, rows=None, T=6)
    got = fcd.crf_spot_batch_raw(_to(device)(p), _to(device)(marg), c["motifs"], c["lens"], track=True, spans=True).cpu()
    assert got.end[0].tolist() == [0, 2] and got.start[0].tolist() == [0, 0], (got.end, got.start)
    assert got.track[0, 1, 2] == got.track[0, 1, 3] > -math.inf  # (the tie is there)
    check(got, c, tie=True)


def run_property(fcd, y, N, device):
    """the reference's v_hit IS the enumerated maximum (1e-12); the kernel's (and crf_spot's) within the bound"""
    x = np.random.default_rng(7 + N).standard_normal((7, 4, N)).astype(np.float32)
    p, marg = TR.transitions64(x)["probs"].astype(np.float32), MR.marginals64(x)["marg"].astype(np.float32)
    ref, want = R.crf_spot(p, marg, y), R.brute_force(p, marg, y)
    assert abs(math.exp(ref["logp"]) - want) <= 1e-12 * want and want > 1e-6, (ref["logp"], want)
    c = dict(name="best_path", p=p[None], marg=marg[None], motifs=np.array([y], np.uint8), lens=np.array([len(y)], np.uint32),
             lengths=None, rows=None, T=7)
    check(fcd.crf_spot_batch_raw(_to(device)(c["p"]), _to(device)(c["marg"]), c["motifs"], c["lens"], track=True, spans=True).cpu(), c)
    if device is None:  # the one-read call from raw scores: its own p and marg, each within a few f32 roundings of these
        one = fcd.crf_spot(x, "".join("NACGT"[v] for v in y), "NAC" if N == 3 else "NACGT")
        assert one[:2] == (ref["first"], ref["end"]) and abs(one[2] - ref["logp"]) <= 1e-4, (one, ref["first"], ref["end"], ref["logp"])


def run_cross(fcd, device):
    """on the ragged case: the spot track never exceeds crf_detect_batch_raw's (max <= sum, by more than both bounds), and the
    located rows are strictly ordered between first and end"""
    c, to = build("ragged_M3"), _to(device)
    args = (to(c["pin"]), to(c["marg"]), c["motifs"], c["lens"], None if c["lengths"] is None else to(c["lengths"]))
    spot, det = fcd.crf_spot_batch_raw(*args, track=True, spans=True).cpu(), fcd.crf_detect_batch_raw(*args, track=True).cpu()
    S, N = c["p"].shape[2:]
    for r, i in np.ndindex(spot.end.shape):
        L, n = int(c["lens"][i]), int(c["lengths"][r])
        h = min(L, R.history(S, N))
        ne = (N - 1) ** (R.history(S, N) - h + 1)
        for t in range(n):
            s, d = float(spot.track[r, i, t]), float(det.track[r, i, t])
            assert s == -math.inf or s <= d + track_bound(t + 1, ne, s) + DC.track_bound(t + 1, ne, d), (r, i, t, s, d)
        if spot.end[r, i] != NO_HIT:
            st = spot.spans.start[r, i, h - 1:L].astype(np.int64)
            assert st[0] == spot.start[r, i] and st[-1] == spot.end[r, i] and (np.diff(st) > 0).all(), (r, i, st)


def run_no_workspace(fcd, c, device):
    """spans=False leaves the handle's workspace at the parameter blocks and logp; spans=True takes the back-pointers"""
    from fast_ctc_decode_amd import _native as nat
    h, to = nat.default_handle(), _to(device)
    args = (to(c["pin"]), to(c["marg"]), c["motifs"], c["lens"], to(c["lengths"]))
    (B, T), M = c["p"].shape[:2], len(c["lens"])
    staged = 0
    if device is None:  # (host arrays are staged in the same workspace: what crf_detect_batch_raw, which has no more, takes)
        h.release_workspace()
        fcd.crf_detect_batch_raw(*args, track=True)
        staged = h.workspace_bytes()
    h.release_workspace()
    got = fcd.crf_spot_batch_raw(*args, track=True, spans=False)
    assert got.spans is None and h.workspace_bytes() <= staged + 4096, (h.workspace_bytes(), staged)  # (end and first: 2 * 4 * B * M more)
    h.release_workspace()
    fcd.crf_spot_batch_raw(*args, spans=True)
    assert h.workspace_bytes() >= staged + B * M * T * 8, (h.workspace_bytes(), staged)
    return got.cpu()


def run_case(fcd, name, device=None):
    k = CASES[name]
    if "prop" in k:
        return run_property(fcd, k["prop"], k["N"], device)
    if k.get("tie"):
        return run_tie(fcd, device)
    if k.get("refusals"):
        return run_refusals()
    if k.get("cross"):
        return run_cross(fcd, device)
    c = build(name)
    if not c["spans"]:
        return check(run_no_workspace(fcd, c, device), c)
    if c["host"] and device is None:  # fcd_crf_spot_host itself, every nullable pointer set (n_valid = 3, 1, 0, 2; rows 0 .. 70)
        rc, msg, got, n_valid = _raw_call(c, every=True)
        assert rc == 0, msg
        return check(got, dict(c, rows=(0, 70)), n_valid)
    pin, marg, lengths = c["pin"], c["marg"], c["lengths"]
    if device is not None:
        import torch
        dev = _to(device)
        pin, marg = (dev(pin.view(np.int16)).view(torch.bfloat16) if c["kw"] else dev(pin)), dev(marg)
        lengths = None if lengths is None else dev(lengths)
    kw = c["kw"] if device is None else {}
    check(fcd.crf_spot_batch_raw(pin, marg, c["motifs"], c["lens"], lengths, c["rows"], track=c["track"], spans=True, **kw).cpu(), c)
