"""TEST INFRASTRUCTURE shared by tests/test_crf_occupancy_wide_emu.py (the kernels on the wave64 emulator) and
tests/test_gpu_crf_occupancy_wide.py (on the GPU): the table of windows beyond 512 states, run through
crf_occupancy_batch_raw(wide=True) and crf_score_batch_raw(wide=True) and compared with the float64 restatement
tests/crf_occupancy_reference.py (occupancy64).  Cases, builder, checker and tolerances are tests/crf_occupancy_cases.py's:
B = 3 reads of lengths (T, T - 3, 0), two labellings per read, a prefilled buffer.  The bound of an entry does not change
with the window's home -- (6 T_r + W + 1) 2^-24 occ, tolerance() of that file -- and lost(T_r, J) takes the J = ceil(states /
64) states a lane holds in K's place (include/fcd.h, fcd_set_crf_lattice_wide).

states(case): the widest window of the call, min(T, y.stride) + 1 or 2 band + 1, what the host sizes J by.
"w_full_ring" brings its own builder: y.stride = 575 labels against T = 1200 rows is a window of 576 = 64 * 9 states, every
slot of the ring live in the rows 574 .. 624, which build_case (y.stride = T) cannot express."""
import math

import numpy as np

import crf_lattice_cases as CC
import crf_occupancy_cases as OC
import crf_occupancy_reference as O
from crf_occupancy_cases import _case

CASES = [
    _case("w_s4n5_t513_l512", 4, 5, 513, 512, 9),        # 514 states: J = 9, the last chunk of the ring nearly empty
    _case("w_s4n5_t1100_l540", 4, 5, 1100, 540, 18),     # 541 live states at mid-read, in a ring of 64 * 18
    _case("w_full_ring", 4, 5, 1200, 575, 9, stride=575),  # 576 states in 64 * 9 slots
    _case("w_s4n5_t1200_l600_band256", 4, 5, 1200, 600, 9, band=256),  # a sliding window of 513 states
    # every state shares two entries, and every row reads the same two posteriors whatever the state: alpha's row is the
    # distribution of a sum of coin tosses, whose tail at 560 labels in 600 rows lies 2^-390 below its mode -- outside any
    # f32 row, and given up.  One label every other row is what such posteriors support: 600 labels in 1200 rows under a
    # band of 256 -- 513 live states colliding in two entries while the window slides round the ring of 576 slots
    _case("w_s4n5_t1200_homopolymer_band256", 4, 5, 1200, 600, 9, band=256, mod="homopolymer"),
    _case("w_s256n5_t520_l515_gathered", 256, 5, 520, 515, 9),  # S N = 1280 > 1024: gathered from global memory
    _case("w_s8n9_t520_l514", 8, 9, 520, 514, 9),               # N - 1 = 8
    _case("w_s4n5_t520_f16_tm", 4, 5, 520, 515, 9, dtype="f16", layout="time", time_major_out=True),
    _case("w_s4n5_t520_accumulate_minus", 4, 5, 520, 515, 9, scale=-1.0, accumulate=True),
    _case("w_s1024n5_t520", 1024, 5, 520, 514, 9),              # the model's size: an S * N row of 20 KiB
    _case("w_s4n5_t520_long_labelling", 4, 5, 520, 515, 9, mod="long"),  # L > T_r
    _case("w_s4n5_t520_zero_row", 4, 5, 520, 515, 9, mod="zero_row"),    # a row of zeros: P = 0
    _case("w_s4n5_t520_nan_row", 4, 5, 520, 515, 9, mod="nan_row"),      # a NaN in a contributing cell
]
EMU_CASES = tuple(CASES)  # (S = 1024 takes the emulator a second: it runs there too)
LAUNCHES = {"crfp_fwd_kernel<8>", "crfp_back_kernel<8,2,4>"}

_built = {}


def states(case):
    exact = min(case["T"], case.get("stride", max(case["T"], 1))) + 1
    return min(exact, 2 * case["band"] + 1) if case["band"] else exact


def states_per_lane(case):
    return -(-states(case) // 64)


def _build_strided(case):
    """crf_occupancy_cases.build_case with the labellings' rows case["stride"] labels long instead of T: the same three reads
    and two labellings each, the same seeds, supports and references"""
    S, N, T, L, stride = case["S"], case["N"], case["T"], case["L"], case["stride"]
    assert L <= stride < T and not case["band"] and not case.get("mod") and case["dtype"] == "f32"
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(case["name"])))
    B, n_hyp = 3, 2
    x = CC.posteriors(rng, B, T, S, N)
    lengths = np.array([T, max(T - 3, 0), 0], np.int64)
    n_valid = np.array([2, 1, 2], np.uint32)
    init = rng.random((B, S)).astype(np.float32)
    labels = np.zeros((B, n_hyp, stride), np.uint8)
    paths = np.zeros((B, n_hyp, stride), np.uint32)
    out_len = np.zeros((B, n_hyp), np.uint32)
    for b in range(B):
        Tr = int(lengths[b])
        n = min(Tr, L)
        y = rng.integers(1, N, n)
        rows = np.sort(rng.choice(max(Tr, 1), n, replace=False))
        for i in range(n_hyp):
            m = max(n - i, 0)
            labels[b, i, :m], paths[b, i, :m], out_len[b, i] = y[:m], rows[:m], m
        if Tr == 0:
            labels[b, 1, 0], out_len[b, 1] = 1, 1
        OC._support(x[b, :Tr], init[b], y, rows)
    refs = {}
    for b in range(B):
        Tr = int(lengths[b])
        for i in range(int(n_valid[b])):
            n = int(out_len[b, i])
            refs[(b, i)] = O.occupancy64(x[b, :Tr], init[b], labels[b, i, :n])
    return dict(case, B=B, n_hyp=n_hyp, xin=x, x32=x, init=init, lengths=lengths, n_valid=n_valid, labels=labels, paths=paths,
                out_len=out_len, refs=refs, pre=None)


def build_case(case):
    """the arrays of a case and the reference of each of its labellings; built once, shared, never changed"""
    if case["name"] not in _built:
        c = _build_strided(case) if case.get("stride") else OC.build_case(case)
        assert states(case) > 512 and states_per_lane(case) == case["k"], (case["name"], states(case))
        _built[case["name"]] = c
    return _built[case["name"]]


def call_args(c, device=None):
    """-> (the positional arguments crf_score_batch_raw and crf_occupancy_batch_raw share, the keywords, conv)"""
    xin, conv, kw = CC._device_inputs(c, device)
    band = c["band"]
    args = (xin, conv(c["init"]), conv(c["labels"]), conv(c["out_len"]), conv(c["lengths"]),
            conv(c["paths"]) if band else None, band, conv(c["n_valid"]))
    return args, kw, conv


def run_case(fcd, c, device=None):
    """crf_occupancy_cases.run_case with wide=True on both calls: the score first (its bits are what the occupancy call's
    logp must hold), then the occupancies into a prefilled buffer.  A labelling of the table that comes back given up fails
    check(): its reference has a value and NaN is within no tolerance."""
    args, kw, _ = call_args(c, device)
    buf, view, before = OC.out_buffer(c)
    score = fcd.crf_score_batch_raw(*args, wide=True, **kw)
    if device is None:
        out = view
    else:
        import torch
        dbuf = torch.from_numpy(buf).to(device)
        out = dbuf.permute(1, 2, 0, 3, 4) if c.get("time_major_out") else dbuf
    got = fcd.crf_occupancy_batch_raw(*args, out=out, scale=c.get("scale", 1.0), accumulate=bool(c.get("accumulate")), wide=True, **kw)
    if device is not None:
        score = score.cpu().numpy()
    got = got.cpu()
    for (b, i), ref in c["refs"].items():
        if ref["occ"] is not None:
            assert math.isfinite(got.logp[b, i]), (c["name"], b, i, "a labelling of the table was given up")
    return OC.check(c, np.asarray(got.occupancy), np.asarray(got.logp), score, before)


# ---- the boundary of what one exponent per row holds, beyond the registers ----
HOLDS = (1500, 700)     # exp(N(0, 1)) posteriors, random labels: a training chunk of an untrained network
GIVEN_UP = (3000, 520)  # uniform random posteriors, six rows per label


def holds(fcd, device=None):
    """(T, L) = HOLDS on a read that does not support its labelling: a finite logp, every row summing to 1 within lost(T_r, J),
    every entry within the relative tolerance plus the mass its row may have lost"""
    to = OC._conv(device)
    rng = np.random.default_rng(43)
    T, L = HOLDS
    J = -(-(T + 1) // 64)
    x = OC._random_posteriors(rng, T, 1.0)[None]
    init = rng.random((1, 4)).astype(np.float32)
    y = np.zeros((1, T), np.uint8)
    y[0, :L] = rng.integers(1, 5, L)
    got = fcd.crf_occupancy_batch_raw(to(x), to(init), to(y), to(np.array([L], np.uint32)), wide=True).cpu()
    ref = O.occupancy64(x[0], init[0], y[0, :L])
    assert math.isfinite(ref["logp"]) and abs(got.logp[0, 0] - ref["logp"]) <= CC.tolerance(T), (T, L, got.logp, ref["logp"])
    occ = np.asarray(got.occupancy)[0, 0].astype(np.float64)
    sums = np.abs(occ.sum(axis=(1, 2)) - 1.0)
    print("crf_occupancy_wide: unsupported (%d, %d): rows sum to 1 within %.3g (lost %.3g)" % (T, L, sums.max(), OC.lost(T, J)))
    assert (sums <= OC.lost(T, J)).all(), (T, L, "rows sum to 1 within lost(T_r)")
    err = np.abs(occ - ref["occ"])
    allow = OC.tolerance(T, L + 1, ref["occ"]) + OC.lost(T, J) + (6.0 * T + L + 2) * 2.0 ** -24
    print("crf_occupancy_wide: unsupported (%d, %d): largest |error| %.3g (absolute allowance %.3g)" % (T, L, err.max(), OC.lost(T, J)))
    assert (err <= allow).all(), (T, L, float((err / allow).max()))


def given_up(fcd, device=None):
    """(T, L) = GIVEN_UP next to a labelling that keeps its value, once written and once accumulated: logp NaN and NaN in
    every row of the block; the other block and its rows t >= T_r as they must be"""
    to = OC._conv(device)
    rng = np.random.default_rng(47)
    T, L = GIVEN_UP
    x = np.stack([OC._random_posteriors(rng, T, 0), OC._random_posteriors(rng, T, 0)])
    init = rng.random((2, 4)).astype(np.float32)
    y = np.zeros((2, L), np.uint8)
    y[0], y[1, :40] = rng.integers(1, 5, L), rng.integers(1, 5, 40)
    lens, lengths = np.array([L, 40], np.uint32), np.array([T, 90], np.int64)
    ref = O.occupancy64(x[1, :90], init[1], y[1, :40])
    J = -(-(L + 1) // 64)
    for accumulate in (False, True):
        buf = np.full((2, 1, T, 4, 5), 0.25, np.float32)
        out = buf if device is None else to(buf)
        got = fcd.crf_occupancy_batch_raw(to(x), to(init), to(y), to(lens), to(lengths), out=out, accumulate=accumulate, wide=True).cpu()
        occ, logp = np.asarray(got.occupancy), np.asarray(got.logp)
        assert math.isnan(logp[0, 0]) and np.isnan(occ[0, 0]).all(), "a lattice the rows cannot hold must be given up"
        base = 0.25 if accumulate else 0.0
        assert abs(logp[1, 0] - ref["logp"]) <= CC.tolerance(90)
        assert (np.abs(occ[1, 0, :90] - base - ref["occ"]) <= OC.tolerance(90, 41, ref["occ"]) + OC.lost(90, J) + 2.0 ** -24).all()
        assert (occ[1, 0, 90:] == 0.25).all()


def workspace_limit_groups(fcd, device=None):
    """a workspace limit of one byte: every read is a launch pair of its own, in the same memory; the same logp bits, the
    occupancies within tolerance of each other's reference (the LDS float adds of colliding entries are unordered)"""
    from fast_ctc_decode_amd import _native as nat
    c = build_case(CASES[0])
    args, kw, _ = call_args(c, device)
    h = nat.default_handle() if device is None else nat.default_handle(0)
    whole = fcd.crf_occupancy_batch_raw(*args, wide=True, **kw).cpu()
    h.set_workspace_limit(1)
    try:
        parts = fcd.crf_occupancy_batch_raw(*args, wide=True, **kw).cpu()
    finally:
        h.set_workspace_limit(0)
    assert np.array_equal(np.asarray(whole.logp).view(np.uint64), np.asarray(parts.logp).view(np.uint64))
    assert np.isfinite(np.asarray(whole.logp)[0]).all()
    zeros = np.zeros((c["B"], c["n_hyp"], c["T"], c["S"], c["N"]), np.float32)
    score = fcd.crf_score_batch_raw(*args, wide=True, **kw)
    score = score if device is None else score.cpu().numpy()
    OC.check(c, np.asarray(parts.occupancy), np.asarray(parts.logp), score, zeros)
