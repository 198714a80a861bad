"""TEST INFRASTRUCTURE shared by tests/test_crf_posterior_emu.py (the kernels on the wave64 emulator) and
tests/test_gpu_crf_posterior.py (on the GPU): seeded cases (built by crf_lattice_cases.build_case) run through
crf_posterior_batch_raw and compared with the float64 restatement tests/crf_posterior_reference.py.

Tolerance: |post - ref| <= 4/3 * (8 T_r + 6) * 2^-24 * ref + 2^-100 -- 4/3 of the bound include/fcd.h derives by counting
roundings along the longest chain (the margin the other lattice walks are tested with), the absolute floor for variants the
contract lets the kernel drop.  logp is held to crf_lattice_cases.tolerance, crf_score's.  A row's sum: N - 1 entries, each
within the tolerance of values that sum to 1, plus the N - 2 float32 roundings of adding them up.

The restatement scores L (N - 1) variants per labelling with a Python loop per cell: where that would run to minutes the
comparison takes a fixed subset of the positions, chosen before anything runs -- both ends of the labelling (where chains
are cut by the end, and state 0), the positions around every multiple of 64 (a lane's, and a ring's, first and last slot)
and every 29th in between.  The reference of a (case, band) is computed once and shared.

A case: crf_lattice_cases' tuple (name, S, N, T, B, n_hyp, dtype, layout, bands, fill).  stride = T, so exact mode at T
rows is a window of T + 1 states whatever the labellings hold: T = 63 / 64 / 127 / 128 / 255 / 256 / 511 are the windows of
64 / 65 / 128 / 129 / 256 / 257 / 512 states, the edges of 1, 2, 4 and 8 states per lane.  S = 4 / 16 / 64 / 1024 at N = 5 are
histories of m = 1 / 2 / 3 / 5 labels (S = 1, where every label but 1 leaves the table, has a test of its own in
tests/test_crf_posterior_emu.py); S * N > 1024 is gathered from global memory."""
import math

import numpy as np

import crf_lattice_cases as CC
import crf_lattice_reference as R
import crf_posterior_reference as PR

CASES = [
    ("w64_s4n5_t63", 4, 5, 63, 1, 1, "f32", "read", (0,), 0.7),
    ("w65_s4n5_t64_f16", 4, 5, 64, 2, 1, "f16", "read", (0, 4), 0.7),
    ("w128_s16n5_t127", 16, 5, 127, 1, 1, "f32", "read", (0,), 0.8),
    ("w129_s4n5_t128_tm", 4, 5, 128, 2, 1, "f32", "time", (0, 64), 0.8),
    ("w256_s16n5_t255", 16, 5, 255, 1, 1, "f32", "read", (0,), 0.85),
    ("w257_s4n5_t256", 4, 5, 256, 1, 1, "f32", "read", (0,), 0.85),
    ("w512_s4n5_t511", 4, 5, 511, 1, 1, "f32", "read", (0,), 0.8),
    ("m1_s4n5_t40_nhyp3", 4, 5, 40, 3, 3, "f32", "read", (0, 1, 4, 64), 0.7),
    ("m2_s16n5_t40_bf16", 16, 5, 40, 2, 1, "bf16", "read", (0, 4), 0.7),
    ("m3_s64n5_t40_tm", 64, 5, 40, 2, 2, "f32", "time", (0, 1, 4), 0.7),
    ("m5_s1024n5_t40_f16", 1024, 5, 40, 2, 1, "f16", "read", (0, 4), 0.7),
    ("m3_s8n3_t40", 8, 3, 40, 2, 1, "f32", "read", (0, 4), 0.6),
    ("m1_s8n9_t40", 8, 9, 40, 2, 1, "f32", "read", (0, 4), 0.6),
    ("m3_s64n5_t200_b64", 64, 5, 200, 1, 1, "f32", "read", (64,), 0.85),
    ("m5_s1024n5_t150_b64", 1024, 5, 150, 1, 1, "f32", "read", (64,), 0.9),
    ("wrap_k1_s4n5_t200", 4, 5, 200, 1, 1, "f32", "read", (4,), 0.8),
]
GPU_CASES = tuple(c[0] for c in CASES)  # the GPU twin runs the same table

build_case = CC.build_case
_refs = {}
worst_seen = {}  # (case, band) -> worst |error| / bound (the bound itself, not the tested 4/3 of it)


def bound(Tr, ref):
    return (8.0 * max(Tr, 1) + 6.0) * 2.0 ** -24 * ref


def tolerance(Tr, ref):
    return 4.0 / 3.0 * bound(Tr, ref) + 2.0 ** -100


def positions(L, N, T):
    """the positions of a labelling the comparison takes: all of them while the restatement stays cheap"""
    if L * L * (N - 1) * T <= 4_000_000:
        return list(range(L))
    pick = set(range(min(L, 8))) | set(range(max(0, L - 8), L)) | set(range(11, L, 29))
    for edge in range(64, L + 2, 64):
        pick |= {k for k in (edge - 2, edge - 1, edge, edge + 1) if 0 <= k < L}
    return sorted(pick)


def reference_one(x, init, y, band, pth, pos=None):
    """-> (positions, post at those positions (n, N-1), logp) of one labelling; pos: the positions to take, where the caller
    has fewer in mind than positions() gives"""
    N = x.shape[2]
    y = [int(v) for v in y]
    pos = positions(len(y), N, x.shape[0]) if pos is None else list(pos)
    logp = R.crf_score(x, init, y, band, pth)
    post = np.full((len(pos), N - 1), math.nan)
    if math.isfinite(logp):
        for j, k in enumerate(pos):
            row = np.array([logp if c == y[k] else R.crf_score(x, init, y[:k] + [c] + y[k + 1:], band, pth) for c in range(1, N)])
            if not np.isnan(row).any() and row.max() > -math.inf:
                w = np.exp(row - row.max())
                post[j] = w / w.sum()
    if len(pos) == len(y):  # (the subset is PR.crf_posterior's own arithmetic: the small cases check that)
        full, lp = PR.crf_posterior(x, init, y, band, pth)
        assert np.array_equal(full, post, equal_nan=True) and (lp == logp or (lp != lp and logp != logp))
    return pos, post, logp


def reference(c, band):
    """{(b, i): (positions, post, logp)} of the case at one band, every scored labelling; computed once"""
    key = (c["name"], band)
    if key not in _refs:
        out = {}
        B, n_hyp = c["out_len"].shape
        for b in range(B):
            Tr = c["T"] if c["lengths"] is None else int(c["lengths"][b])
            for i in range(n_hyp if c["n_valid"] is None else min(n_hyp, int(c["n_valid"][b]))):
                n = int(c["out_len"][b, i])
                pth = c["paths"][b, i, :n] if band else None
                out[(b, i)] = reference_one(c["x32"][b, :Tr], c["init"][b], c["labels"][b, i, :n], band, pth)
        _refs[key] = out
    return _refs[key]


def check_one(got, ref, Tr, what):
    """one labelling's post rows (n, N-1) against the restatement's; returns worst |error| / bound"""
    assert got.shape == ref.shape, what
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN where the restatement has a value, or the reverse", got, ref)
    if nan.all():
        return 0.0
    err = np.abs(got - ref)[~nan]
    ratio = err / tolerance(Tr, ref[~nan])
    frac = float((err / np.maximum(bound(Tr, ref[~nan]), 2.0 ** -100)).max())
    print("crf_posterior:", what, "T_r", Tr, "worst |error| / bound = %.3f" % frac)
    assert ratio.max() <= 1.0, (what, "T_r", Tr, "worst |error| / tolerance", ratio.max())
    sums = got.sum(-1)[~nan.any(-1)]
    assert np.all(np.abs(sums - 1.0) <= tolerance(Tr, 1.0) + got.shape[1] * 2.0 ** -24), (what, "rows sum to 1", sums)
    return frac


def check(got, c, band):
    """got: PosteriorResult on numpy"""
    B, n_hyp = c["out_len"].shape
    N = c["N"]
    assert got.post.dtype == np.float32 and got.post.shape == (B, n_hyp, c["labels"].shape[2], N - 1)
    assert got.logp.dtype == np.float64 and got.logp.shape == (B, n_hyp)
    refs = reference(c, band)
    worst = 0.0
    for b in range(B):
        Tr = c["T"] if c["lengths"] is None else int(c["lengths"][b])
        for i in range(n_hyp):
            n = int(c["out_len"][b, i])
            if c["n_valid"] is not None and i >= int(c["n_valid"][b]):
                assert got.logp[b, i] != got.logp[b, i], ("rows that are no hypothesis are NaN", b, i)
                assert np.isnan(got.post[b, i, :n]).all() and (got.post[b, i, n:] == 0).all()
                continue
            pos, post, lp = refs[(b, i)]
            assert math.isfinite(lp), (c["name"], band, b, i, "the case is meant to have an alignment")
            assert abs(got.logp[b, i] - lp) <= CC.tolerance(Tr), (c["name"], band, b, i, got.logp[b, i], lp)
            worst = max(worst, check_one(got.post[b, i, pos], post, Tr, (c["name"], "band", band, b, i)))
            assert np.isfinite(got.post[b, i, :n]).all() and (got.post[b, i, n:] == 0).all()
    worst_seen[(c["name"], band)] = worst
    return worst


def run_case(fcd, c, device=None):
    """the case at each of its bands (numpy through _host, or torch tensors on `device` through _dev) against the
    restatement; logp is crf_score_batch_raw's value bit for bit (the same forward recurrence)"""
    xin, conv, kw = CC._device_inputs(c, device)
    for band in c["bands"]:
        args = (xin, conv(c["init"]), conv(c["labels"]), conv(c["out_len"]), conv(c["lengths"]),
                conv(c["paths"]) if band else None, band, conv(c["n_valid"]))
        got = fcd.crf_posterior_batch_raw(*args, **kw)
        score = fcd.crf_score_batch_raw(*args, **kw)
        if device is not None:
            assert got.post.device == xin.device and got.logp.device == xin.device
            score = score.cpu().numpy()
        got = got.cpu()
        assert np.array_equal(got.logp, score, equal_nan=True), (c["name"], band)
        check(got, c, band)


def edge_batch():
    """-> (x, init, labels, lens, lengths): the edge rows of include/fcd.h, S = 4, N = 5
    0: L = 0   1: T_r = 0, L = 0   2: T_r = 0, L > 0   3: L > T_r   4: label N   5: label 0   6: a NaN y itself reads
    7: L = T_r   8: an ordinary row   9: len > stride   10: a NaN that only a variant reads   11: a NaN, but L > T_r first"""
    rng = np.random.default_rng(4)
    B = 12
    x = CC.posteriors(rng, B, 6, 4, 5)
    init = np.tile(np.array([0.1, 0.7, 0.7, 0.2], np.float32), (B, 1))  # sigma_0 = 1, the FIRST maximum
    labels = np.zeros((B, 8), np.uint8)
    lens = np.zeros(B, np.uint32)
    lengths = np.full(B, 6, np.int64)
    lengths[1] = lengths[2] = 0
    labels[2, :1], lens[2] = [1], 1
    labels[3, :7], lens[3] = [1, 2, 1, 2, 1, 2, 1], 7
    labels[4, :2], lens[4] = [1, 5], 2
    labels[5, :2], lens[5] = [2, 0], 2
    labels[6, :2], lens[6] = [3, 1], 2  # sigma = 1, 2, 0
    x[6, 3, 2, 0] = np.nan
    labels[7, :6], lens[7] = [1, 2, 3, 4, 1, 2], 6
    labels[8, :3], lens[8] = [1, 1, 3], 3
    labels[9, :], lens[9] = 1, 9
    labels[10, :2], lens[10] = [3, 1], 2  # the variant [4, 1] stays in model state 3 over row 1; nothing else reads that
    x[10, 1, 3, 0] = np.nan
    labels[11, :7], lens[11] = [1, 2, 1, 2, 1, 2, 1], 7
    x[11, 2, 1, 0] = np.nan
    return x, init, labels, lens, lengths


def check_edges(post, logp, x, init, labels, lens, lengths, unwritten):
    """post (12, 8, 4), logp (12,) of edge_batch(); entries the call must not write hold `unwritten`"""
    lp = logp
    assert abs(lp[0] - np.log(x[0, :, 1, 0].astype(np.float64)).sum()) <= 6 * 2.0 ** -24 and lp[1] == 0.0
    assert lp[2] == -math.inf and lp[3] == -math.inf and lp[11] == -math.inf
    assert all(math.isnan(lp[b]) for b in (4, 5, 6, 9))
    for b in range(12):
        n = min(int(lens[b]), 8)
        if b in (7, 8, 10):
            ref, rlp = PR.crf_posterior(x[b], init[b], labels[b, :n])
            assert math.isfinite(rlp) and abs(lp[b] - rlp) <= CC.tolerance(6), b
            check_one(post[b, :n], ref, 6, "edge row %d" % b)
            if b == 10:
                assert np.isnan(post[b, 0]).all() and np.isfinite(post[b, 1]).all()
        else:
            assert np.isnan(post[b, :n]).all(), (b, post[b, :n])
        assert (post[b, n:] == unwritten).all(), (b, "entries k >= len", post[b, n:])


# ---- cases outside the table, shared by the emulator file and its GPU twin (device=None: numpy through _host) ----
def _conv(device):
    if device is None:
        return lambda a: a
    import torch
    return lambda a: None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device)


def _posterior(fcd, device, x, init, labels, lens, lengths=None, paths=None, band=0):
    to = _conv(device)
    got = fcd.crf_posterior_batch_raw(to(x), to(init), to(labels), to(lens), to(lengths), to(paths) if band else None, band)
    return got.cpu()


def chains_cut_by_the_end(fcd, S, N, device=None):
    """L <= m, and k + m >= L for every k: no chain of the labelling reaches the state where it would rejoin"""
    rng = np.random.default_rng(50 + S + N)
    T, B = 9, 7
    x = CC.posteriors(rng, B, T, S, N)
    init = rng.random((B, S)).astype(np.float32)
    labels = np.zeros((B, T), np.uint8)
    lens = np.arange(B).astype(np.uint32) + 1  # L = 1 .. 7
    for b in range(B):
        labels[b, :lens[b]] = rng.integers(1, N, lens[b])
    got = _posterior(fcd, device, x, init, labels, lens)
    for b in range(B):
        n = int(lens[b])
        ref, lp = PR.crf_posterior(x[b], init[b], labels[b, :n])
        assert abs(got.logp[b, 0] - lp) <= CC.tolerance(T)
        check_one(got.post[b, 0, :n], ref, T, ("short", S, N, "L", n))


def single_state_model(fcd, device=None):
    """S = 1: sigma_{k+1} = y_k - 1 is the table's one row after label 1 and outside it after any other -- a labelling of
    1s (the last label free: a state entered at the last row reads nothing) has alignments, a variant with another label
    before the last row has none, and a labelling with a 2 inside has no posterior at all"""
    rng = np.random.default_rng(70)
    T, B = 20, 4
    x = CC.posteriors(rng, B, T, 1, 5)
    init = np.ones((B, 1), np.float32)
    labels = np.zeros((B, T), np.uint8)
    lens = np.array([1, 6, 12, 5], np.uint32)
    for b in range(B):
        labels[b, :lens[b]] = 1
    labels[1, 5], labels[2, 11] = 3, 4
    labels[3, 2] = 2
    got = _posterior(fcd, device, x, init, labels, lens)
    for b in range(B):
        n = int(lens[b])
        ref, lp = PR.crf_posterior(x[b], init[b], labels[b, :n])
        assert math.isfinite(lp) == (b != 3) and (got.logp[b, 0] == lp or abs(got.logp[b, 0] - lp) <= CC.tolerance(T))
        check_one(got.post[b, 0, :n], ref, T, ("S = 1", b))
        if b != 3 and n > 1:
            assert (got.post[b, 0, :n - 1, 1:] == 0).all() and (got.post[b, 0, n - 1] > 0).all()


def band_against_both_cuts(fcd, band, device=None):
    """paths that emit everything at once: k(t) runs ahead of what is reachable (the k <= t + 1 cut holds the window), or
    stays behind what must be reached (the k >= L - (T_r - 1 - t) cut does); and an ordinary path"""
    rng = np.random.default_rng(60 + band)
    T, L = 30, 12
    x = CC.posteriors(rng, 3, T, 4, 5)
    init = rng.random((3, 4)).astype(np.float32)
    labels = np.zeros((3, T), np.uint8)
    labels[:, :L] = rng.integers(1, 5, (3, L))
    paths = np.zeros((3, T), np.uint32)
    paths[0, :L] = np.arange(L) // 3            # three labels a row at the start
    paths[1, :L] = T - 1 - (L - 1 - np.arange(L)) // 3  # three labels a row at the end
    paths[2, :L] = np.sort(rng.choice(T, L, replace=False))
    lens = np.full(3, L, np.uint32)
    got = _posterior(fcd, device, x, init, labels, lens, None, paths, band)
    finite = 0
    for b in range(3):
        ref, lp = PR.crf_posterior(x[b], init[b], labels[b, :L], band, paths[b, :L])
        if math.isfinite(lp):
            assert abs(got.logp[b, 0] - lp) <= CC.tolerance(T)
            finite += 1
        else:
            assert got.logp[b, 0] == lp
        check_one(got.post[b, 0, :L], ref, T, ("cuts", band, b))
    assert finite >= 1


def heavy_variants(fcd, device=None):
    """variants that outweigh the called labelling by more than f32 has exponent: the accumulators' own exponent holds them.
    Read 0: T = 8, y = [2, 3, 1] from sigma_0 = 0 walks the rows 0, 1, 2, 0; label 3 has 1e-30 in row 1 at every t and the
    whole of row 2 is scaled by 1e-12, so every variant of position 0 or 1 -- it reads other rows -- is heavier than y by
    more than 2^130.  Read 1 (T_r = 4, y = [1]): sigma_0 = 2, whose row holds 1e-20 for the stay and 2e-38 for label 1; nothing
    is emitted at the last row, and row 0 -- the model state after label 1 only -- is scaled by 1e-6."""
    rng = np.random.default_rng(80)
    x = CC.posteriors(rng, 2, 8, 4, 5)
    init = np.array([[0.9, 0.1, 0.2, 0.3], [0.1, 0.2, 0.9, 0.3]], np.float32)  # sigma_0 = 0, 2
    labels = np.zeros((2, 8), np.uint8)
    labels[0, :3], labels[1, :1] = [2, 3, 1], [1]
    lens = np.array([3, 1], np.uint32)
    lengths = np.array([8, 4], np.int64)
    x[0, :, 1, 3] = 1e-30
    x[0, :, 2, :] *= np.float32(1e-12)
    x[1, :, 2, 0], x[1, :, 2, 1] = 1e-20, 2e-38
    x[1, 3, 2, 1:] = 0.0
    x[1, :, 0, :] *= np.float32(1e-6)
    got = _posterior(fcd, device, x, init, labels, lens, lengths)
    for b in range(2):
        n, Tr = int(lens[b]), int(lengths[b])
        sub, lp = PR.crf_substitutions(x[b, :Tr], init[b], labels[b, :n])
        ref, _ = PR.crf_posterior(x[b, :Tr], init[b], labels[b, :n])
        assert math.isfinite(lp) and sub.max() - lp > 130 * math.log(2.0), ("the case is meant to be lopsided", b, sub, lp)
        assert np.isfinite(ref).all() and abs(got.logp[b, 0] - lp) <= CC.tolerance(Tr)
        check_one(got.post[b, 0, :n], ref, Tr, ("heavy variants", b))


def workspace_limit_groups(fcd, device=None):
    """a workspace limit of one byte: every read is a launch pair of its own, in the same memory; the same values"""
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(8)
    to = _conv(device)
    x = CC.posteriors(rng, 6, 40, 16, 5)
    init = rng.random((6, 16)).astype(np.float32)
    lengths = np.array([40, 17, 40, 1, 33, 40], np.int64)
    h = nat.default_handle() if device is None else nat.default_handle(0)
    r = fcd.crf_beam_search_batch_raw(to(x), to(init), 5, 0.0, lengths=to(lengths))
    nb = fcd.crf_beam_search_nbest_batch_raw(to(x[:3]), to(init[:3]), 2, beam_size=5, lengths=to(lengths[:3]))
    for res, xs, ins, ls in ((r, x, init, lengths), (nb, x[:3], init[:3], lengths[:3])):
        for band in (0, 4):
            whole = res.crf_posterior(to(xs), to(ins), lengths=to(ls), band=band).cpu()
            h.set_workspace_limit(1)
            try:
                parts = res.crf_posterior(to(xs), to(ins), lengths=to(ls), band=band).cpu()
            finally:
                h.set_workspace_limit(0)
            assert np.array_equal(whole.post, parts.post, equal_nan=True) and np.array_equal(whole.logp, parts.logp, equal_nan=True)
            assert np.isfinite(whole.logp[:, 0]).all()
