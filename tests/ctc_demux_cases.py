"""TEST INFRASTRUCTURE of tests/test_ctc_demux_emu.py and tests/test_gpu_ctc_demux.py: ctc_detect_batch_raw(packed=True)
(fcd_set_ctc_detect_packed, one (read, motif) pair per lane) against the float64 statement tests/ctc_detect_reference.py
per (read, motif), at the smallest shapes at which the packing can go wrong.  Posteriors k / 4096 (exact in f16):
background 256 .. 768 from the case's seed, planted labels 3680.  Asserted from the reference's own numbers, as
tests/ctc_detect_cases.py does: the best c_t leads the runner-up by 1 + 2^-12 (the tie case: a tie required), then end is
exact; count within (3 n + 4) 2^-24 relatively, logp absolutely, for a range of n rows -- that file's bound: the packed
cell is the same two adds and one multiply, the weights the same roundings, the rescaling by powers of two only."""

import numpy as np
import pytest

import ctc_align_cases as AC
import ctc_detect_cases as DC
import ctc_detect_reference as R

CAP, NO_HIT = 24, 0xFFFFFFFF
_M24 = DC._M24
_MANY = [[1 + (i >> (2 * k)) % 4 for k in range(2 + i % 3)] for i in range(65)]  # 65 motifs of 2 .. 4 labels
_RAGGED = dict(B=9, T=60, motifs=[[1, 2, 3], [4, 2], _M24[:7]], lengths=[60, 0, 33, 7, 60, 41, 2, 18, 60],
               plant=[(0, 0, 50), (2, 1, 20), (2, 2, 25), (3, 0, 2), (4, 2, 1), (5, 0, 36), (7, 1, 15), (8, 0, 57)])
CASES = {
    "reads_65_motifs_1": dict(B=65, T=20, motifs=[[1, 2, 3]], plant=[(r, 0, r % 17) for r in range(65)]),
    "padded_lanes_motifs_3": dict(B=17, T=20, motifs=[[1, 2], [3, 4, 1], [2]], plant=[(r, r % 3, r % 15) for r in range(17)]),
    "one_read_blocks_motifs_64": dict(B=2, T=70, motifs=_MANY[:64], plant=[(0, 5, 3), (1, 63, 66)]),
    "second_block_motifs_65": dict(B=2, T=12, motifs=_MANY, plant=[(0, 64, 3), (1, 0, 7)]),
    "lengths_0_1_2_cap": dict(B=3, T=40, motifs=[[], [3], [2, 4], _M24], plant=[(0, 3, 9), (1, 2, 30), (2, 1, 0)]),
    "repeats": dict(B=2, T=9, motifs=[[1, 1], [1, 2, 1]], plant=[(0, 1, 2), (1, 0, 4)]),
    "repeats_nocollapse": dict(B=2, T=9, motifs=[[1, 1], [1, 2, 1]], plant=[(0, 1, 2), (1, 0, 4)], collapse=False),
    "ragged_head": dict(_RAGGED, rows=(5, 40)),
    "ragged_tail": dict(_RAGGED, rows=(-30, None)),
    "short_and_empty_ranges": dict(_RAGGED, rows=(30, 34)),
    "nan_in_one_read": dict(B=4, T=30, motifs=[[1, 2, 3], [4, 1]], rows=(4, 24), plant=[(r, r % 2, 10) for r in range(4)],
                            nan=[(1, 12), (2, 27)]),  # (read 1: inside its range; read 2: outside, changes nothing)
    "exponent_200_rows_of_0.9": dict(B=2, T=200, motifs=[[1, 2], _M24, [3, 3]], plant=[], const=0.9),
    "f16": dict(B=3, T=40, motifs=[_M24, [2, 1]], plant=[(0, 0, 3), (1, 1, 20), (2, 0, 16)], dtype="f16"),
    "time_major": dict(B=3, T=40, motifs=[_M24, [2, 1]], plant=[(0, 0, 3), (1, 1, 20), (2, 0, 16)], time_major=True),
    "tie_halves": dict(B=1, T=6, N=3, motifs=[[1], [2, 1]], plant=[], matrix=DC._HALVES),
}


def build(name):
    k = CASES[name]
    B, T, N, motifs = k["B"], k["T"], k.get("N", 5), k["motifs"]
    rng = np.random.default_rng(k.get("seed", 0))
    x = rng.integers(256, 769, (B, T, N)).astype(np.float32) / 4096
    for r, i, t in k["plant"]:
        for j, y in enumerate(motifs[i]):
            x[r, t + j, y] = 230 / 256
    if "const" in k:
        x[:] = k["const"]
    if "matrix" in k:
        x = np.array([k["matrix"]], np.float32)
    for r, t in k.get("nan", []):
        x[r, t, 2] = np.nan
    stride = max(max(map(len, motifs)), 1)
    xin = x.astype(np.float16) if k.get("dtype") == "f16" else x
    if k.get("time_major"):
        xin = np.ascontiguousarray(xin.transpose(1, 0, 2)).transpose(1, 0, 2)
    return dict(name=name, x32=xin.astype(np.float32), xin=xin, dtype=k.get("dtype", "f32"), T=T, rows=k.get("rows"),
                motifs=np.array([m + [0] * (stride - len(m)) for m in motifs], np.uint8), lens=np.array(list(map(len, motifs)), np.uint32),
                lengths=None if "lengths" not in k else np.array(k["lengths"], np.int64), collapse=k.get("collapse", True))


_refs = {}


def reference(name):
    """the case and its float64 results per (read, motif), computed once"""
    if name not in _refs:
        c, ref = build(name), {}
        for r in range(c["x32"].shape[0]):
            Tr = c["T"] if c["lengths"] is None else int(c["lengths"][r])
            b, e, _ = slice(*(c["rows"] or (None, None))).indices(Tr)
            for i, L in enumerate(c["lens"]):
                ref[r, i] = (R.ctc_detect(c["x32"][r, :Tr], c["motifs"][i, :L], c["collapse"], b, e), max(e - b, 0))
        _refs[name] = (c, ref)
    return _refs[name]


def check(got, name):
    c, refs = reference(name)
    assert got.track is None and got.end.shape == (c["x32"].shape[0], len(c["lens"]))
    for (r, i), (ref, n) in refs.items():
        where = (name, r, i)
        if ref["end"] is not None:  # the condition on the inputs
            best = sorted(ref["c"])[::-1]
            if "matrix" in CASES[name] and i == 0:
                assert best[0] == best[1] and ref["c"].index(best[0]) == ref["end"], where + ("no tie in the tie case",)
            else:
                assert len(best) == 1 or best[0] >= best[1] * (1 + 2.0 ** -12), where + tuple(best[:2])
        count, logp = float(got.count[r, i]), float(got.logp[r, i])
        print(where, "count", count, ref["count"], "logp", logp, ref["logp"], "end", got.end[r, i], ref["end"])
        assert DC.close(count, ref["count"], DC.bound(n) * ref["count"] if ref["end"] is not None else 0.0), where + (count, ref["count"])
        assert DC.close(logp, ref["logp"], DC.bound(n)), where + (logp, ref["logp"])
        assert got.end[r, i] == (NO_HIT if ref["end"] is None else ref["end"]), where + (got.end[r, i], ref["end"])


def call(fcd, c, device=None, **kw):
    xin, conv, more = AC._device_inputs(c, device)
    return fcd.ctc_detect_batch_raw(xin, c["motifs"], c["lens"], c["collapse"], conv(c["lengths"]), c["rows"], **more, **kw).cpu()


def run_refusals(fcd, device=None):
    c = reference("f16")[0]
    with pytest.raises(ValueError, match="track"):
        call(fcd, c, device, packed=True, track=True)
    long = dict(c, motifs=np.ones((1, CAP + 1), np.uint8), lens=np.array([CAP + 1], np.uint32))
    with pytest.raises(RuntimeError, match="beyond %d labels" % CAP):
        call(fcd, long, device, packed=True)


def run_packed_against_unpacked(fcd, device=None):
    """the same input through both walks: equal end, both within their bounds of the reference"""
    c = reference("ragged_head")[0]
    packed, plain = call(fcd, c, device, packed=True), call(fcd, c, device)
    check(packed, "ragged_head")
    check(fcd.DetectResult(plain.count, plain.end, plain.logp, None), "ragged_head")
    assert np.array_equal(packed.end, plain.end)
    print("bit-identical count:", np.array_equal(packed.count, plain.count, equal_nan=True),
          "logp:", np.array_equal(packed.logp, plain.logp, equal_nan=True))


NAMES = sorted(CASES) + ["refusals", "packed_against_unpacked"]


def run_case(fcd, name, device=None):
    if name not in CASES:
        return {"refusals": run_refusals, "packed_against_unpacked": run_packed_against_unpacked}[name](fcd, device)
    check(call(fcd, reference(name)[0], device, packed=True), name)
