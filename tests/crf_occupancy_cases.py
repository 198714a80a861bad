"""TEST INFRASTRUCTURE shared by tests/test_crf_occupancy_emu.py (the kernels on the wave64 emulator) and
tests/test_gpu_crf_occupancy.py (on the GPU): one table of seeded cases run through crf_occupancy_batch_raw and compared with
the float64 restatement tests/crf_occupancy_reference.py (occupancy64).

Every case has B = 3 reads of lengths (T, max(T - 3, 0), 0) and n_hyp = 2 labellings per read with n_valid = (2, 1, 2):
a full read, a ragged one, an empty one, and a block that is no hypothesis.  The caller's buffer is prefilled -- with 77 where
the call writes (accumulate = 0), with seeded values where it adds -- so that everything the call must not touch shows:
rows t >= T_r, blocks without a positive finite P(y | x), blocks of i >= n_valid.

Tolerance of an entry: 4/3 * (6 T_r + W + 2) * 2^-24 * occ + 2^-100 with W the window's states (L + 1, or 2 band + 1 if that
is fewer): 4/3 of the roundings along the longest chain -- alpha_{t-1} 3 t, beta_t 3 (T_r - 1 - t), the term 3, P 3 T_r and
its mantissa 1, an entry's sum W - 1 -- and the floor below which the contract lets a term go.  Accumulate mode adds
2^-24 |out| for the final sum (scale = -1 and 0.5 multiply exactly).  A row's entries sum to scale within the sum of
their tolerances (the sum is taken in float64).  logp must equal crf_score_batch_raw's bits.

A case: dict(name, S, N, T, L, dtype, layout, band, k, and optionally scale / accumulate / time_major_out / pad / mod)."""
import math

import numpy as np

import crf_lattice_cases as CC
import crf_lattice_reference as R
import crf_occupancy_reference as O

FILL = np.float32(77.0)


def _case(name, S, N, T, L, k, dtype="f32", layout="read", band=0, **kw):
    return dict(name=name, S=S, N=N, T=T, L=L, k=k, dtype=dtype, layout=layout, band=band, **kw)


CASES = [
    _case("s4n5_t1_l0", 4, 5, 1, 0, 1),
    _case("s4n5_t1_l1", 4, 5, 1, 1, 1),
    _case("s4n5_t7_homopolymer", 4, 5, 7, 5, 1, mod="homopolymer"),  # every state shares two entries: the collision path
    _case("s4n5_t70_k2", 4, 5, 70, 66, 2),
    _case("s4n5_t140_k4", 4, 5, 140, 130, 4),
    _case("s4n5_t330_k8", 4, 5, 330, 300, 8),
    _case("s4n5_t130_band4", 4, 5, 130, 60, 1, band=4),  # crosses the tile (51 rows at S N = 20) where k(t) is refilled
    _case("s16n5_t12", 16, 5, 12, 8, 1),
    _case("s64n5_t10_f16_tm", 64, 5, 10, 6, 1, dtype="f16", layout="time", time_major_out=True),
    _case("s256n5_t9_gathered", 256, 5, 9, 5, 1),  # S N = 1280 > 1024: the posteriors are gathered, not staged
    _case("s1024n3_t8_bf16_padded", 1024, 3, 8, 5, 1, dtype="bf16", pad=7),
    _case("s3n2_t8", 3, 2, 8, 4, 1),
    _case("s5n4_t9_dead_end", 5, 4, 9, 4, 1, mod="dead_end"),  # no power of nb; sigma leaves the table: logp = -inf
    _case("s4n5_t7_accumulate_minus", 4, 5, 7, 4, 1, scale=-1.0, accumulate=True),
    _case("s4n5_t7_accumulate_half", 4, 5, 7, 4, 1, scale=0.5, accumulate=True),
    _case("s4n5_t7_zero_row", 4, 5, 7, 4, 1, mod="zero_row"),  # a row of zeros: P = 0
    _case("s4n5_t7_nan_row", 4, 5, 7, 4, 1, mod="nan_row"),    # a NaN in a contributing cell
    _case("s4n5_t7_long_labelling", 4, 5, 7, 4, 1, mod="long"),  # L > T_r
]
GPU_CASES = tuple(c["name"] for c in CASES)  # the GPU twin runs the same table

worst_seen = {}  # case -> the largest |error| / tolerance over its entries
_built = {}


def _support(x, init, y, rows):
    """Make the read support its labelling, as the read a labelling was decoded from does: the posterior of the edge the
    alignment `rows` takes at each row is raised eightfold and its (t, s) row renormalised.  The walks keep one exponent per
    row, and a cell below 2^-160 of its row's maximum may be dropped (include/fcd.h): an entry's tolerance has the absolute
    floor 2^-100 on the premise that such a cell carries less than that -- true where alpha's and beta's row maxima meet on
    the alignments that carry the probability, not for a labelling its read does not support (uniform random posteriors and
    300 labels in 330 rows put the two maxima at opposite ends of the cone, 2^-370 of their product apart from P)."""
    T, S, N = x.shape
    sig = R.trajectory(init, y, S, N)
    k = 0
    for t in range(T):
        emit = k < len(rows) and rows[k] == t
        if 0 <= sig[k] < S:
            x[t, sig[k], int(y[k]) if emit else 0] *= 8.0
            x[t, sig[k]] /= x[t, sig[k]].sum()
        k += int(emit)


def build_case(case):
    """the arrays of a case and the reference of each of its labellings; built once, shared, never changed"""
    if case["name"] in _built:
        return _built[case["name"]]
    S, N, T, L, band = case["S"], case["N"], case["T"], case["L"], case["band"]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(case["name"])))
    B, n_hyp = 3, 2
    x = CC.posteriors(rng, B, T, S, N)
    mod = case.get("mod")
    lengths = np.array([T, max(T - 3, 0), 0], np.int64)
    n_valid = np.array([2, 1, 2], np.uint32)
    init = rng.random((B, S)).astype(np.float32)
    if mod == "dead_end":  # sigma_0 = 3, label 3: (3 * 3) mod 5 + 2 = 6, outside the table, with a label still to emit
        init[0] = [0.1, 0.2, 0.3, 0.9, 0.4]
    stride = max(T, 1) + (1 if mod == "long" else 0)
    labels = np.zeros((B, n_hyp, stride), np.uint8)
    paths = np.zeros((B, n_hyp, stride), np.uint32)
    out_len = np.zeros((B, n_hyp), np.uint32)
    for b in range(B):
        Tr = int(lengths[b])
        n = min(Tr, L)
        y = np.full(n, 2) if mod == "homopolymer" else rng.integers(1, N, n)
        rows = np.sort(rng.choice(max(Tr, 1), n, replace=False))
        if mod == "dead_end" and b == 0:
            y[:2] = [3, 1]
        # the second labelling: the first without its last label, emitted at the same rows
        for i in range(n_hyp):
            m = max(n - i, 0)
            labels[b, i, :m], paths[b, i, :m], out_len[b, i] = y[:m], rows[:m], m
        if mod == "long" and b == 1:
            labels[b, 0, :Tr + 1], out_len[b, 0] = rng.integers(1, N, Tr + 1), Tr + 1
        if Tr == 0:
            labels[b, 1, 0], out_len[b, 1] = 1, 1  # (T_r = 0: L = 0 has logp 0 and no row to write, L = 1 has no alignment)
        _support(x[b, :Tr], init[b], y, rows)
    if mod == "zero_row":
        x[0, T // 2] = 0.0
    if mod == "nan_row":
        x[0, 1] = np.nan
    if case["dtype"] == "f16":
        xin = x.astype(np.float16)
        x32 = xin.astype(np.float32)
    elif case["dtype"] == "bf16":
        bits = (x.view(np.uint32) >> 16).astype(np.uint16)  # truncation: any bf16 value will do
        xin, x32 = bits, (bits.astype(np.uint32) << 16).view(np.float32)
    else:
        xin = x32 = x
    if case["layout"] == "time":
        xin = np.ascontiguousarray(xin.transpose(1, 0, 2, 3)).transpose(1, 0, 2, 3)
    if case.get("pad"):  # one more state row than the model has: stride_t = (S + 1) N
        big = np.zeros((B, T, S + 1, N), xin.dtype)
        big[:, :, :S] = xin
        xin = big[:, :, :S]
    refs = {}
    for b in range(B):
        Tr = int(lengths[b])
        for i in range(int(n_valid[b])):
            n = int(out_len[b, i])
            refs[(b, i)] = O.occupancy64(x32[b, :Tr], init[b], labels[b, i, :n], band, paths[b, i, :n] if band else None)
    if mod == "dead_end":
        assert refs[(0, 0)]["logp"] == -math.inf
    if mod == "zero_row":
        assert refs[(0, 0)]["logp"] == -math.inf and refs[(0, 1)]["logp"] == -math.inf
    if mod == "nan_row":
        assert math.isnan(refs[(0, 0)]["logp"]) and math.isnan(refs[(0, 1)]["logp"])
    if mod == "long":
        assert refs[(1, 0)]["logp"] == -math.inf
    if mod is None:
        assert refs[(0, 0)]["occ"] is not None and refs[(0, 1)]["occ"] is not None and refs[(1, 0)]["occ"] is not None or T < 4
    pre = None
    if case.get("accumulate"):
        pre = rng.standard_normal((B, n_hyp, T, S, N)).astype(np.float32)
    c = dict(case, B=B, n_hyp=n_hyp, xin=xin, x32=x32, init=init, lengths=lengths, n_valid=n_valid, labels=labels, paths=paths,
             out_len=out_len, refs=refs, pre=pre)
    _built[case["name"]] = c
    return c


def bound(Tr, W, occ):
    return (6.0 * Tr + W + 2.0) * 2.0 ** -24 * occ


def tolerance(Tr, W, occ):
    return 4.0 / 3.0 * bound(Tr, W, occ) + 2.0 ** -100


def out_buffer(c):
    """-> (the numpy buffer as the caller allocates it, its (B, n_hyp, T, S, N) view, what every entry holds before)"""
    B, n_hyp, T, S, N = c["B"], c["n_hyp"], c["T"], c["S"], c["N"]
    before = c["pre"] if c["pre"] is not None else np.full((B, n_hyp, T, S, N), FILL, np.float32)
    if c.get("time_major_out"):
        buf = np.ascontiguousarray(before.transpose(2, 0, 1, 3, 4))
        return buf, buf.transpose(1, 2, 0, 3, 4), before
    if c.get("pad"):  # rows c["pad"] floats apart
        buf = np.full((B, n_hyp, T, S * N + c["pad"]), FILL, np.float32)
        view = np.lib.stride_tricks.as_strided(buf, (B, n_hyp, T, S, N), buf.strides[:3] + (N * 4, 4))
        view[...] = before
        return buf, view, before
    buf = before.copy()
    return buf, buf, before


def check(c, occ, logp, score, before):
    """occ (B, n_hyp, T, S, N) float32 and logp (B, n_hyp) as numpy arrays, score: crf_score_batch_raw's (B, n_hyp)"""
    B, n_hyp, T, S, N = c["B"], c["n_hyp"], c["T"], c["S"], c["N"]
    scale = np.float32(c.get("scale", 1.0))
    acc = bool(c.get("accumulate"))
    assert occ.shape == (B, n_hyp, T, S, N) and occ.dtype == np.float32
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
            assert abs(logp[b, i] - ref["logp"]) <= CC.tolerance(Tr), (c["name"], b, i, logp[b, i], ref["logp"])
            assert same[Tr:].all(), (c["name"], b, i, "rows t >= T_r were touched")
            n = int(c["out_len"][b, i])
            W = min(n + 1, 2 * c["band"] + 1) if c["band"] else n + 1
            want = ref["occ"]
            tol = tolerance(Tr, W, want)
            got = occ[b, i, :Tr].astype(np.float64)
            if acc:
                held = before[b, i, :Tr].astype(np.float64)
                tol = np.where(want > 0, tol + 2.0 ** -24 * np.abs(got), 0.0)  # (an entry of occupancy 0 is not touched)
                got = (got - held) / float(scale)
                tol = tol / abs(float(scale))
                assert (occ[b, i, :Tr][want == 0].view(np.uint32) == before[b, i, :Tr][want == 0].view(np.uint32)).all()
            else:
                got = got / float(scale)
            err = np.abs(got - want)
            assert (err <= tol).all(), (c["name"], b, i, "T_r", Tr, "W", W, "worst |error| / tolerance",
                                        float((err / np.maximum(tol, 2.0 ** -100)).max()))
            sums = got.sum(axis=(1, 2))
            assert (np.abs(sums - 1.0) <= tol.sum(axis=(1, 2))).all(), (c["name"], b, i, "rows sum to scale", sums)
            worst = max(worst, float((err / np.maximum(tol, 2.0 ** -100)).max(initial=0.0)))
    worst_seen[c["name"]] = worst
    print("crf_occupancy: %s worst |error| / tolerance = %.3f" % (c["name"], worst))
    return worst


def run_case(fcd, c, device=None):
    """the case through crf_occupancy_batch_raw into a prefilled buffer: numpy through _host, or torch tensors on `device`
    through _dev"""
    xin, conv, kw = CC._device_inputs(c, device)
    band = c["band"]
    buf, view, before = out_buffer(c)
    args = (xin, conv(c["init"]), conv(c["labels"]), conv(c["out_len"]), conv(c["lengths"]),
            conv(c["paths"]) if band else None, band, conv(c["n_valid"]))
    score = fcd.crf_score_batch_raw(*args, **kw)
    if device is None:
        out = view
    else:
        import torch
        dbuf = torch.from_numpy(buf).to(device)
        if c.get("time_major_out"):
            out = dbuf.permute(1, 2, 0, 3, 4)
        elif c.get("pad"):
            out = torch.as_strided(dbuf, view.shape, tuple(s // 4 for s in view.strides))
        else:
            out = dbuf
    got = fcd.crf_occupancy_batch_raw(*args, out=out, scale=c.get("scale", 1.0), accumulate=bool(c.get("accumulate")), **kw)
    if device is not None:
        assert got.occupancy.device == xin.device and got.logp.device == xin.device
        score = score.cpu().numpy()
        if c.get("pad"):  # the padding between the rows keeps its fill
            assert (dbuf.cpu().numpy()[..., c["S"] * c["N"]:] == FILL).all()
    elif c.get("pad"):
        assert (buf[..., c["S"] * c["N"]:] == FILL).all()
    got = got.cpu()
    return check(c, np.asarray(got.occupancy), got.logp, score, before)


def lost(Tr, K):
    """include/fcd.h, lost(T_r): how far from 1 the walk lets a row's terms sum before it gives the labelling up"""
    return 2.0 * (6.0 * Tr + 64 * K + 2 * K + 8) * 2.0 ** -24


def _random_posteriors(rng, T, spread):
    """(T, 4, 5) posteriors no labelling is supported by: uniform random (spread 0) or exp(spread * N(0, 1)), rows normalised"""
    x = rng.random((T, 4, 5)) if spread == 0 else np.exp(spread * rng.standard_normal((T, 4, 5)))
    return (x / x.sum(-1, keepdims=True)).astype(np.float32)


def unsupported_labellings(fcd, device=None):
    """The boundary of what rows with one float32 exponent hold (include/fcd.h), on reads that do NOT support their
    labellings -- random labels against random posteriors, S = 4, N = 5, exact lattice.  Inside it: a finite logp, every
    row summing to 1 within lost(T_r), every entry within the relative tolerance plus the mass its row may have lost,
    lost(T_r) + (6 T_r + W + 1) 2^-24 absolute.  (T, L) = (330, 300): the widest cone the 512 states take at these lengths;
    (600, 300) and (1000, 330), posteriors spread by exp(N(0, 1)): training chunks of an untrained network.  Beyond it --
    (1500, 127), five times more rows than the cone is wide -- the walk gives the labelling up: logp NaN and NaN in every
    row of its block, written or accumulated; the labelling next to it in the batch keeps its value."""
    to = _conv(device)
    rng = np.random.default_rng(41)
    for T, L, spread, K in ((330, 300, 0, 8), (600, 300, 1.0, 8), (1000, 330, 1.0, 8)):
        x = _random_posteriors(rng, T, spread)[None]
        init = rng.random((1, 4)).astype(np.float32)
        y = rng.integers(1, 5, (1, L)).astype(np.uint8)
        got = fcd.crf_occupancy_batch_raw(to(x), to(init), to(y), to(np.array([L], np.uint32))).cpu()
        ref = O.occupancy64(x[0], init[0], y[0])
        assert math.isfinite(ref["logp"]) and abs(got.logp[0, 0] - ref["logp"]) <= CC.tolerance(T), (T, L, got.logp, ref["logp"])
        occ = got.occupancy[0, 0].astype(np.float64)
        assert (np.abs(occ.sum(axis=(1, 2)) - 1.0) <= lost(T, K)).all(), (T, L, "rows sum to 1 within lost(T_r)")
        err = np.abs(occ - ref["occ"])
        allow = tolerance(T, L + 1, ref["occ"]) + lost(T, K) + (6.0 * T + L + 2) * 2.0 ** -24
        print("crf_occupancy: unsupported (%d, %d): largest |error| %.3g (absolute allowance %.3g), largest relative error of the "
              "entries above 1e-6: %.3g" % (T, L, err.max(), lost(T, K), (err / np.maximum(ref["occ"], 1e-300))[ref["occ"] > 1e-6].max()))
        assert (err <= allow).all(), (T, L, float((err / allow).max()))
    # beyond the boundary, next to a labelling inside it; once written, once accumulated onto a prefilled buffer
    T = 1500
    x = np.stack([_random_posteriors(rng, T, 0), _random_posteriors(rng, T, 0)])
    init = rng.random((2, 4)).astype(np.float32)
    y = np.zeros((2, 127), np.uint8)
    y[0], y[1, :40] = rng.integers(1, 5, 127), rng.integers(1, 5, 40)
    lens, lengths = np.array([127, 40], np.uint32), np.array([T, 90], np.int64)
    for accumulate in (False, True):
        buf = np.full((2, 1, T, 4, 5), 0.25, np.float32)
        out = buf if device is None else to(buf)
        got = fcd.crf_occupancy_batch_raw(to(x), to(init), to(y), to(lens), to(lengths), out=out, accumulate=accumulate).cpu()
        assert math.isnan(got.logp[0, 0]) and np.isnan(got.occupancy[0, 0]).all(), "a lattice the rows cannot hold must be given up"
        ref = O.occupancy64(x[1, :90], init[1], y[1, :40])
        base = 0.25 if accumulate else 0.0
        assert abs(got.logp[1, 0] - ref["logp"]) <= CC.tolerance(90)
        assert (np.abs(got.occupancy[1, 0, :90] - base - ref["occ"]) <= tolerance(90, 41, ref["occ"]) + lost(90, 1) + 2.0 ** -24).all()
        assert (got.occupancy[1, 0, 90:] == 0.25).all()


def _conv(device):
    if device is None:
        return lambda a: a
    import torch
    return lambda a: None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device)


def workspace_limit_groups(fcd, device=None):
    """a workspace limit of one byte: every read is a launch pair of its own, in the same memory; the same bits"""
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(9)
    to = _conv(device)
    x = CC.posteriors(rng, 5, 30, 16, 5)
    init = rng.random((5, 16)).astype(np.float32)
    lengths = np.array([30, 17, 30, 1, 22], np.int64)
    h = nat.default_handle() if device is None else nat.default_handle(0)
    r = fcd.crf_beam_search_nbest_batch_raw(to(x), to(init), 2, beam_size=5, lengths=to(lengths))
    for band in (0, 4):
        whole = r.crf_occupancy(to(x), to(init), lengths=to(lengths), band=band).cpu()
        h.set_workspace_limit(1)
        try:
            parts = r.crf_occupancy(to(x), to(init), lengths=to(lengths), band=band).cpu()
        finally:
            h.set_workspace_limit(0)
        assert np.array_equal(whole.occupancy, parts.occupancy) and np.array_equal(whole.logp, parts.logp, equal_nan=True)
        assert np.isfinite(whole.logp[:, 0]).all() and whole.occupancy.shape == (5, 2, 30, 16, 5)
        rc = r.cpu()
        for b in (0, 1, 4):
            n, Tr = int(rc.out_len[b, 0]), int(lengths[b])
            ref = O.occupancy64(x[b, :Tr], init[b], rc.labels[b, 0, :n], band, rc.path[b, 0, :n] if band else None)
            W = min(n + 1, 2 * band + 1) if band else n + 1
            assert (np.abs(whole.occupancy[b, 0, :Tr] - ref["occ"]) <= tolerance(Tr, W, ref["occ"])).all()
            assert (whole.occupancy[b, 0, Tr:] == 0).all()
