"""TEST INFRASTRUCTURE shared by tests/test_ctc_occupancy_emu.py (the kernels on the wave64 emulator) and
tests/test_gpu_ctc_occupancy.py (on the GPU): one table of seeded cases run through ctc_occupancy_batch_raw and compared with
the float64 restatement tests/ctc_occupancy_reference.py (occupancy64).

Every case has B = 3 reads of lengths (T, max(T - 3, 0), 0) and n_hyp = 2 labellings per read with n_valid = (2, 1, 2):
a full read, a ragged one, an empty one, and a block that is no hypothesis.  The caller's buffer is prefilled -- with 77 where
the call writes (accumulate = 0), with seeded values (or the posteriors themselves: the softmax buffer of a training step)
where it adds -- so that everything the call must not touch shows: rows t >= T_r, blocks without a positive finite
P(y | x), blocks of i >= n_valid.

Tolerance of an entry, include/fcd.h's formulae and nothing looser:  |occ - ref| <= bound(T_r) * ref + lost(T_r)  with
bound(T_r) = (6 T_r + K / 2 + 11) 2^-24 and lost(T_r) = 2 (6 T_r + K / 2 + 19) 2^-24, K the states a lane holds.  Accumulate
mode adds 2^-24 |out| for the final sum (scale = -1 and 0.5 multiply exactly).  A row's entries sum to 1 within lost(T_r)
(the sum is taken in float64).  logp must equal ctc_score_batch_raw's bits.

A case: dict(name, N, T, L, k, collapse, dtype, layout, band and optionally stride / scale / accumulate / time_major_out /
pad / mod).  The labels' stride is L where the case does not say (the window's states, and with them K, follow min(T, stride)):
K = 2 holds min(T, stride) <= 62 exactly, 4 <= 126, 6 <= 190, 8 <= 254; the 63 and 127 labels of the issue's list land in
K = 4 and 6, so 62 and 126 stand beside them and every K runs."""
import math

import numpy as np

import ctc_occupancy_reference as O
import ctc_score_cases as SC

FILL = np.float32(77.0)


def _case(name, N, T, L, k, collapse=True, dtype="f32", layout="read", band=0, **kw):
    return dict(name=name, N=N, T=T, L=L, k=k, collapse=collapse, dtype=dtype, layout=layout, band=band, **kw)


CASES = [
    _case("n5_t1_l0", 5, 1, 0, 2),
    _case("n5_t1_l1", 5, 1, 1, 2),
    _case("n5_t9_l9_one_alignment", 5, 9, 9, 2),  # read 0: T = L, occ is one-hot
    _case("n3_t5_homopolymer", 3, 5, 3, 2, mod="homopolymer"),  # [1,1,1] in 5 rows: the blanks are forced
    _case("n3_t6_homopolymer", 3, 6, 3, 2, mod="homopolymer"),  # read 1 (3 rows): the repeats need 5, P = 0
    _case("n3_t5_homopolymer_nocollapse", 3, 5, 3, 2, collapse=False, mod="homopolymer"),
    _case("n3_t6_homopolymer_nocollapse", 3, 6, 3, 2, collapse=False, mod="homopolymer"),
    _case("n5_t7_long_labelling", 5, 7, 4, 2, stride=8, mod="long"),  # L > T_r
    _case("n5_t65_l62_k2", 5, 65, 62, 2, mod="peaky"),
    _case("n5_t66_l63_k4", 5, 66, 63, 4, mod="peaky"),
    _case("n9_t129_l126_k4", 9, 129, 126, 4, mod="peaky"),
    _case("n5_t130_l127_k6", 5, 130, 127, 6, mod="peaky"),
    _case("n9_t193_l190_k6", 9, 193, 190, 6, mod="peaky"),
    _case("n5_t257_l254_k8", 5, 257, 254, 8, mod="peaky"),
    _case("n5_t130_band4", 5, 130, 60, 2, band=4),  # crosses the tile (64 rows) where k(t) is refilled
    _case("n9_t130_band4", 9, 130, 60, 2, band=4),
    _case("n2_t130_band4", 2, 130, 60, 2, band=4),
    _case("n5_t130_band4_nocollapse", 5, 130, 60, 2, collapse=False, band=4),
    _case("n5_t260_band_jump", 5, 260, 200, 2, band=4, mod="jump"),  # 200 labels in 3 rows: the window jumps past itself, P = 0
    _case("n5_t40_f16_tm", 5, 40, 17, 2, dtype="f16", layout="time", time_major_out=True),
    _case("n9_t40_bf16_padded", 9, 40, 17, 2, dtype="bf16", pad=7),
    _case("n5_t12_nan_on", 5, 12, 5, 2, mod="nan_on"),    # a NaN on the labelling's alignments
    _case("n5_t12_nan_off", 5, 12, 5, 2, mod="nan_off"),  # ... in the column of a label it does not hold
    _case("n5_t12_bad_label", 5, 12, 5, 2, mod="bad_label"),
    _case("n5_t12_zero_row", 5, 12, 5, 2, mod="zero_row"),  # a row of zeros: P = 0
    _case("n5_t12_accumulate_softmax", 5, 12, 5, 2, scale=-1.0, accumulate=True, mod="softmax"),
    _case("n5_t12_accumulate_half", 5, 12, 5, 2, scale=0.5, accumulate=True),
    _case("n5_t12_scale_minus", 5, 12, 5, 2, scale=-1.0),
]
GPU_CASES = tuple(c["name"] for c in CASES)  # the GPU twin runs the same table

worst_seen = {}
_built = {}


def states_per_lane(T, stride, band):
    """csrc/ctc_posterior.hip, reg_states_per_lane"""
    states = 2 * min(T, stride) + 1
    if band:
        states = min(states, 4 * band + 3)
    return 2 if states + 2 <= 128 else 4 if states + 2 <= 256 else 6 if states + 2 <= 384 else 8


def bound(Tr, K):
    """include/fcd.h, bound(T_r): the relative error of an entry"""
    return (6.0 * Tr + K / 2 + 11) * 2.0 ** -24


def lost(Tr, K):
    """include/fcd.h, lost(T_r): how far from 1 the walk lets a row's sum be before it gives the labelling up"""
    return 2.0 * (6.0 * Tr + K / 2 + 19) * 2.0 ** -24


def tolerance(Tr, K, ref):
    return bound(Tr, K) * ref + lost(Tr, K)


def _labelling(rng, N, n, mod):
    if mod == "homopolymer":
        return np.full(n, 1)
    hi = N - 1 if mod == "nan_off" and N > 2 else N  # (nan_off: label N - 1 stays out)
    y = rng.integers(1, hi, n)
    if mod == "peaky" or N > 2:  # no repeats side by side (where the alphabet allows): n labels fit n rows
        for k in range(1, n):
            while hi > 2 and y[k] == y[k - 1]:
                y[k] = rng.integers(1, hi)
    return y


def build_case(case):
    """the arrays of a case and the reference of each of its labellings; built once, shared, never changed"""
    if case["name"] in _built:
        return _built[case["name"]]
    N, T, L, band, mod = case["N"], case["T"], case["L"], case["band"], case.get("mod")
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(case["name"])))
    B, n_hyp = 3, 2
    x = SC.posteriors(rng, B, T, N)
    lengths = np.array([T, max(T - 3, 0), 0], np.int64)
    n_valid = np.array([2, 1, 2], np.uint32)
    stride = case.get("stride", max(L, 1))
    assert states_per_lane(T, stride, band) == case["k"], (case["name"], states_per_lane(T, stride, band))
    labels = np.zeros((B, n_hyp, stride), np.uint8)
    paths = np.zeros((B, n_hyp, stride), np.uint32)
    out_len = np.zeros((B, n_hyp), np.uint32)
    for b in range(B):
        Tr = int(lengths[b])
        n = min(Tr, L)
        y = _labelling(rng, N, n, mod)
        rows = np.sort(rng.choice(max(Tr, 1), n, replace=False))
        if mod == "jump":  # 67 + 67 + 66 labels at three rows in the middle of the read
            rows = np.repeat([Tr // 2, Tr // 2 + 1, Tr // 2 + 2], [67, 67, 66])[:n]
        # the second labelling: the first without its last label, emitted at the same rows
        for i in range(n_hyp):
            m = max(n - i, 0)
            labels[b, i, :m], paths[b, i, :m], out_len[b, i] = y[:m], rows[:m], m
        if mod == "long" and b == 1:
            labels[b, 0, :Tr + 1], out_len[b, 0] = _labelling(rng, N, Tr + 1, None), Tr + 1
        if Tr == 0:
            labels[b, 1, 0], out_len[b, 1] = 1, 1  # (T_r = 0: L = 0 has logp 0 and no row to write, L = 1 has no alignment)
        if mod == "peaky":  # the read supports its labelling: the symbol the alignment `rows` emits is raised eightfold
            emit = np.zeros(Tr, np.int64)
            emit[rows] = y
            x[b, np.arange(Tr), emit] *= 8.0
            x[b, :Tr] /= x[b, :Tr].sum(-1, keepdims=True)
    if mod == "zero_row":
        x[0, T // 2] = 0.0
    if mod == "nan_on":
        x[0, 1, 0] = np.nan
    if mod == "nan_off":
        x[0, 1, N - 1] = np.nan
    if mod == "bad_label":
        labels[0, 0, 1] = N
    if case["dtype"] == "f16":
        xin = x.astype(np.float16)
        x32 = xin.astype(np.float32)
    elif case["dtype"] == "bf16":
        xin = SC.to_bf16_bits(x)
        x32 = SC.bf16_bits_to_f32(xin)
    else:
        xin = x32 = x
    if case["layout"] == "time":
        xin = np.ascontiguousarray(xin.transpose(1, 0, 2)).transpose(1, 0, 2)
    if case.get("pad"):  # rows pad elements apart: stride_t = N + pad
        big = np.zeros((B, T, N + case["pad"]), xin.dtype)
        big[:, :, :N] = xin
        xin = big[:, :, :N]
    refs = {}
    for b in range(B):
        Tr = int(lengths[b])
        for i in range(int(n_valid[b])):
            n = int(out_len[b, i])
            refs[(b, i)] = O.occupancy64(x32[b, :Tr], labels[b, i, :n], case["collapse"], band, paths[b, i, :n] if band else None)
    # the case holds what its name says
    if mod in ("zero_row", "jump"):
        assert refs[(0, 0)]["logp"] == -math.inf and refs[(0, 1)]["logp"] == -math.inf
    if mod in ("nan_on", "bad_label"):
        assert math.isnan(refs[(0, 0)]["logp"])
    if mod == "long":
        assert refs[(1, 0)]["logp"] == -math.inf
    if mod == "homopolymer" and case["collapse"] and T == 6:
        assert refs[(1, 0)]["logp"] == -math.inf and refs[(0, 0)]["occ"] is not None
    if mod in (None, "peaky", "nan_off", "softmax") and T >= 4:
        assert refs[(0, 0)]["occ"] is not None and refs[(0, 1)]["occ"] is not None and refs[(1, 0)]["occ"] is not None, case["name"]
    if case["name"] == "n5_t9_l9_one_alignment":
        assert np.abs(refs[(0, 0)]["occ"] - refs[(0, 0)]["occ"].round()).max() <= 1e-12  # one-hot
    pre = None
    if mod == "softmax":
        pre = np.repeat(x32[:, None], n_hyp, axis=1).copy()
    elif case.get("accumulate"):
        pre = rng.standard_normal((B, n_hyp, T, N)).astype(np.float32)
    c = dict(case, B=B, n_hyp=n_hyp, stride=stride, xin=xin, x32=x32, lengths=lengths, n_valid=n_valid, labels=labels, paths=paths,
             out_len=out_len, refs=refs, pre=pre)
    _built[case["name"]] = c
    return c


def out_buffer(c):
    """-> (the numpy buffer as the caller allocates it, its (B, n_hyp, T, N) view, what every entry holds before)"""
    B, n_hyp, T, N = c["B"], c["n_hyp"], c["T"], c["N"]
    before = c["pre"] if c["pre"] is not None else np.full((B, n_hyp, T, N), FILL, np.float32)
    if c.get("time_major_out"):
        buf = np.ascontiguousarray(before.transpose(2, 0, 1, 3))
        return buf, buf.transpose(1, 2, 0, 3), before
    if c.get("pad"):  # rows c["pad"] floats apart
        buf = np.full((B, n_hyp, T, N + c["pad"]), FILL, np.float32)
        view = buf[..., :N]
        view[...] = before
        return buf, view, before
    buf = before.copy()
    return buf, buf, before


def check(c, occ, logp, score, before):
    """occ (B, n_hyp, T, N) float32 and logp (B, n_hyp) as numpy arrays, score: ctc_score_batch_raw's (B, n_hyp)"""
    B, n_hyp, T, N, K = c["B"], c["n_hyp"], c["T"], c["N"], c["k"]
    scale = np.float32(c.get("scale", 1.0))
    acc = bool(c.get("accumulate"))
    assert occ.shape == (B, n_hyp, T, N) and occ.dtype == np.float32
    assert logp.shape == (B, n_hyp) and logp.dtype == np.float64
    assert np.array_equal(logp.view(np.uint64), np.asarray(score, np.float64).view(np.uint64)), (c["name"], logp, score)
    worst = 0.0
    for b in range(B):
        Tr = int(c["lengths"][b])
        for i in range(n_hyp):
            same = occ[b, i].view(np.uint32) == before[b, i].view(np.uint32)
            if i >= int(c["n_valid"][b]):
                assert math.isnan(logp[b, i]) and same.all(), (c["name"], b, i, "a block that is no hypothesis was touched")
                continue
            ref = c["refs"][(b, i)]
            if ref["occ"] is None:
                assert (logp[b, i] == ref["logp"]) or (math.isnan(logp[b, i]) and math.isnan(ref["logp"])), (c["name"], b, i)
                assert same.all(), (c["name"], b, i, "a block without a value was touched")
                continue
            assert SC.same(logp[b, i], ref["logp"], Tr), (c["name"], b, i, logp[b, i], ref["logp"])
            assert same[Tr:].all(), (c["name"], b, i, "rows t >= T_r were touched")
            want = ref["occ"]
            tol = tolerance(Tr, K, want)
            got = occ[b, i, :Tr].astype(np.float64)
            if acc:
                held = before[b, i, :Tr].astype(np.float64)
                tol = tol + 2.0 ** -24 * np.abs(got)
                got = (got - held) / float(scale)
                tol = tol / abs(float(scale))
                # (an entry of occupancy 0 is not touched: a label the labelling does not hold)
                absent = np.ones(N, bool)
                absent[[0] + [int(v) for v in c["labels"][b, i, :int(c["out_len"][b, i])]]] = False
                assert same[:Tr][:, absent].all(), (c["name"], b, i, "a cell of occupancy 0 was written")
            else:
                assert not np.signbit(occ[b, i, :Tr][want == 0]).any(), (c["name"], b, i, "a cell of occupancy 0 holds -0")
                got = got / float(scale)
            err = np.abs(got - want)
            assert (err <= tol).all(), (c["name"], b, i, "T_r", Tr, "worst |error| / tolerance", float((err / tol).max()))
            sums = got.sum(axis=1)
            room = lost(Tr, K) + (tol - tolerance(Tr, K, want)).sum(axis=1)  # (accumulate: the final sums' roundings)
            assert (np.abs(sums - 1.0) <= room).all(), (c["name"], b, i, "rows sum to 1", sums)
            worst = max(worst, float((err / tol).max(initial=0.0)))
    worst_seen[c["name"]] = worst
    print("ctc_occupancy: %s worst |error| / tolerance = %.3f" % (c["name"], worst))
    return worst


def _device_inputs(c, device):
    kw = {}
    if device is None:
        if c["dtype"] == "bf16":
            kw["input_dtype"] = "bfloat16"
        return c["xin"], (lambda a: a), kw
    import torch
    xin = c["xin"]
    if c["dtype"] == "bf16":
        full = xin.base if c.get("pad") else xin
        t = torch.from_numpy(np.ascontiguousarray(full).view(np.int16)).to(device).view(torch.bfloat16)
    else:
        t = torch.from_numpy(np.ascontiguousarray(xin.base if c.get("pad") else xin)).to(device)
    if c.get("pad"):
        t = t[..., :c["N"]]
    if c["layout"] == "time":  # time-major on the device too
        t = t.transpose(0, 1).contiguous().transpose(0, 1)
    return t, _conv(device), kw


def run_case(fcd, c, device=None):
    """the case through ctc_occupancy_batch_raw into a prefilled buffer: numpy through _host, or torch tensors on `device`
    through _dev"""
    xin, conv, kw = _device_inputs(c, device)
    band = c["band"]
    buf, view, before = out_buffer(c)
    args = (xin, conv(c["labels"]), conv(c["out_len"]), c["collapse"], conv(c["lengths"]),
            conv(c["paths"]) if band else None, band, conv(c["n_valid"]))
    score = fcd.ctc_score_batch_raw(*args, **kw)
    if device is None:
        out = view
    else:
        import torch
        dbuf = torch.from_numpy(buf).to(device)
        if c.get("time_major_out"):
            out = dbuf.permute(1, 2, 0, 3)
        elif c.get("pad"):
            out = dbuf[..., :c["N"]]
        else:
            out = dbuf
    got = fcd.ctc_occupancy_batch_raw(*args, out=out, scale=c.get("scale", 1.0), accumulate=bool(c.get("accumulate")), **kw)
    if device is not None:
        assert got.occupancy.device == xin.device and got.logp.device == xin.device
        score = score.cpu().numpy()
        if c.get("pad"):  # the padding between the rows keeps its fill
            assert (dbuf.cpu().numpy()[..., c["N"]:] == FILL).all()
    elif c.get("pad"):
        assert (buf[..., c["N"]:] == FILL).all()
    got = got.cpu()
    return check(c, np.asarray(got.occupancy), got.logp, score, before)


def _conv(device):
    if device is None:
        return lambda a: a
    import torch
    return lambda a: None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device)


HELD, GIVEN_UP = (500, 50), (1000, 50)  # (T, L), N = 5, uniform random posteriors, exact lattice: confirmed on the emulator


def unsupported_labellings(fcd, device=None):
    """The boundary of what rows with one float32 exponent hold (include/fcd.h), on reads that do NOT support their
    labellings -- random labels against uniform random posteriors, N = 5, exact lattice (K = 2).  Inside it, 50 labels in
    500 rows: a finite logp, every row summing to 1 within lost(T_r), every entry within bound * ref + lost.  Beyond it,
    50 labels in 1000 rows: the walk gives the labelling up -- logp NaN and NaN in every row of its block, written or
    accumulated; the labelling next to it in the batch keeps its value."""
    to = _conv(device)
    rng = np.random.default_rng(41)

    def uniform(T):
        x = rng.random((T, 5))
        return (x / x.sum(-1, keepdims=True)).astype(np.float32)
    T, L = HELD
    x, y = uniform(T)[None], rng.integers(1, 5, (1, L)).astype(np.uint8)
    got = fcd.ctc_occupancy_batch_raw(to(x), to(y), to(np.array([L], np.uint32))).cpu()
    ref = O.occupancy64(x[0], y[0])
    assert SC.same(got.logp[0, 0], ref["logp"], T), (got.logp, ref["logp"])
    occ = got.occupancy[0, 0].astype(np.float64)
    assert (np.abs(occ.sum(axis=1) - 1.0) <= lost(T, 2)).all(), "rows sum to 1 within lost(T_r)"
    err = np.abs(occ - ref["occ"])
    print("ctc_occupancy: held (%d, %d): largest |error| %.3g, lost %.3g" % (T, L, err.max(), lost(T, 2)))
    assert (err <= tolerance(T, 2, ref["occ"])).all(), float((err / tolerance(T, 2, ref["occ"])).max())
    # beyond the boundary, next to a labelling inside it; once written, once accumulated onto a prefilled buffer
    T, L = GIVEN_UP
    x = np.stack([uniform(T), uniform(T)])
    y = rng.integers(1, 5, (2, L)).astype(np.uint8)
    lens, lengths = np.array([L, 20], np.uint32), np.array([T, 90], np.int64)
    for accumulate in (False, True):
        buf = np.full((2, 1, T, 5), 0.25, np.float32)
        out = buf if device is None else to(buf)
        got = fcd.ctc_occupancy_batch_raw(to(x), to(y), to(lens), True, to(lengths), out=out, accumulate=accumulate).cpu()
        assert math.isnan(got.logp[0, 0]) and np.isnan(got.occupancy[0, 0]).all(), "a lattice the rows cannot hold must be given up"
        ref = O.occupancy64(x[1, :90], y[1, :20])
        base = 0.25 if accumulate else 0.0
        assert SC.same(got.logp[1, 0], ref["logp"], 90)
        assert (np.abs(got.occupancy[1, 0, :90] - base - ref["occ"]) <= tolerance(90, 2, ref["occ"]) + 2.0 ** -24).all()
        assert (got.occupancy[1, 0, 90:] == 0.25).all()


def workspace_limit_groups(fcd, device=None):
    """a workspace limit of one byte: every read is a launch pair of its own, in the same memory; the same bits"""
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(9)
    to = _conv(device)
    x = SC.posteriors(rng, 5, 30, 5)
    lengths = np.array([30, 17, 30, 1, 22], np.int64)
    h = nat.default_handle() if device is None else nat.default_handle(0)
    r = fcd.beam_search_nbest_batch_raw(to(x), 2, 5, 0.0, lengths=to(lengths))
    for band in (0, 4):
        whole = r.ctc_occupancy(to(x), lengths=to(lengths), band=band).cpu()
        h.set_workspace_limit(1)
        try:
            parts = r.ctc_occupancy(to(x), lengths=to(lengths), band=band).cpu()
        finally:
            h.set_workspace_limit(0)
        assert np.array_equal(whole.occupancy, parts.occupancy) and np.array_equal(whole.logp, parts.logp, equal_nan=True)
        assert np.isfinite(whole.logp[:, 0]).all() and whole.occupancy.shape == (5, 2, 30, 5)
        rc = r.cpu()
        K = states_per_lane(30, rc.labels.shape[2], band)
        for b in (0, 1, 4):
            n, Tr = int(rc.out_len[b, 0]), int(lengths[b])
            ref = O.occupancy64(x[b, :Tr], rc.labels[b, 0, :n], True, band, rc.path[b, 0, :n] if band else None)
            assert (np.abs(whole.occupancy[b, 0, :Tr] - ref["occ"]) <= tolerance(Tr, K, ref["occ"])).all()
            assert (whole.occupancy[b, 0, Tr:] == 0).all()
