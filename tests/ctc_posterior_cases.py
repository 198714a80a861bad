"""TEST INFRASTRUCTURE shared by tests/test_ctc_posterior_emu.py (the kernels on the wave64 emulator) and
tests/test_gpu_ctc_posterior.py (on the GPU): the cases of tests/ctc_score_cases.py that fit the limits of
fcd_ctc_posterior_* (windows up to 510 states, N - 1 <= 8) and the comparison of ctc_posterior_batch_raw with the float64
restatement tests/ctc_posterior_reference.py.

Tolerance: |post - ref| <= 16 * T_r * 2^-24 * ref + 2^-100.  alpha at row t - 1 and beta at row t together carry at most
three f32 roundings per row of the read, the w recurrence two per row (the sum of the exits and the stay, the product),
the sum over t one per row: each sub[k][c] has a relative error of at most about 6 T_r 2^-24, a ratio of two such sums
12 T_r 2^-24; 16 leaves room for the second-order terms.  The absolute floor is for variants the contract lets the kernel
drop.  logp is held to ctc_score_cases.tolerance.  Condition on the inputs, asserted per labelling as
ctc_score_cases.check does.

Two properties compare rounded results with one another and get the room that takes.  Band against exact mode: two
kernel results, each within the tolerance of the same exact value, differ by at most twice the tolerance.  A row's sum:
N - 1 entries, each within the tolerance of values that sum to 1 -- together the tolerance at ref = 1 -- plus the
N - 2 float32 roundings of adding them up, (N - 1) 2^-24 at most.

The table is ctc_score_cases.CASES' register-tier rows at their T, raggedness and bands (B and n_hyp trimmed where the
restatement's L * (N - 1) float64 scorings per labelling and band would run to minutes; it is computed once per (case,
band) and shared), with N = 7 raised to 9, plus 9-label alphabets at 2, 4 and 8 states per lane: every
post_back_kernel<K, NC> runs."""
import math

import numpy as np

import ctc_posterior_reference as PR
import ctc_score_cases as SC
import ctc_score_reference as R

# (name, N, T, B, n_hyp, dtype, time_major, collapse, ragged, bands) as ctc_score_cases.CASES
#   windows: bands 1 / 4 / 16 -> 7 / 19 / 67 states (2 per lane; labels enter and leave the window mid-walk), band 64 -> 259
#   (6 per lane where the exact lattice is no smaller), exact 2 T + 1: 19, 81, 121 (2), 201, 221 (4), 341 (6), 391, 461 (8)
CASES = [
    ("n2-tiny", 2, 9, 5, 2, "f32", False, True, True, (0, 1, 4)),
    ("n5-regs2", 5, 40, 6, 3, "f32", False, True, True, (0, 1, 4, 64)),
    ("n5-nocollapse", 5, 60, 3, 5, "f32", False, False, True, (0, 1, 4, 64)),
    ("n5-regs4-f16", 5, 110, 3, 1, "f16", False, True, False, (0, 4, 16)),
    ("n9-regs6-bf16", 9, 170, 2, 1, "bf16", False, True, True, (0, 4, 64)),
    ("n4-regs8-timemajor", 4, 230, 3, 1, "f32", True, True, True, (0, 1, 64)),
    ("n9-regs2-nocollapse", 9, 40, 3, 2, "f32", False, False, True, (0, 1, 4)),
    ("n9-regs4", 9, 100, 1, 1, "f32", False, True, False, (0,)),
    ("n9-regs8-f16", 9, 195, 1, 1, "f16", True, True, False, (0,)),
]

build_case = SC.build_case
_refs = {}


def tolerance(Tr, ref):
    return 16.0 * max(Tr, 1) * 2.0 ** -24 * ref + 2.0 ** -100


def reference(c, band):
    """{(b, i): (post (L, N-1), logp)} of the case at one band, every scored labelling; computed once"""
    key = (c["name"], band)
    if key not in _refs:
        out = {}
        B, n_hyp = c["out_len"].shape
        for b in range(B):
            Tr = c["T"] if c["lengths"] is None else int(c["lengths"][b])
            for i in range(min(n_hyp, int(c["n_valid"][b]))):
                n = int(c["out_len"][b, i])
                y, pth = c["labels"][b, i, :n], (c["paths"][b, i, :n] if band else None)
                x = c["x32"][b, :Tr]
                post, lp = PR.ctc_posterior(x, y, c["collapse"], band, pth)
                cond = R.ctc_logp(x, y, c["collapse"], band, pth, drop=2.0 ** -160)
                assert (lp == cond) or abs(lp - cond) <= 1e-9, ("the case relies on dropped mass", b, i, lp, cond)
                out[(b, i)] = (post, lp)
        _refs[key] = out
    return _refs[key]


def check_one(got, ref, Tr, what):
    """one labelling's post (L, N-1) against the restatement's; returns worst |error| / tolerance"""
    assert got.shape == ref.shape, what
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN where the restatement has a value, or the reverse")
    if nan.all():
        return 0.0
    ratio = np.abs(got - ref)[~nan] / tolerance(Tr, ref[~nan])
    assert ratio.max() <= 1.0, (what, "T_r", Tr, "worst |error| / tolerance", ratio.max())
    sums = got.sum(-1)[~nan.any(-1)]
    assert np.all(np.abs(sums - 1.0) <= tolerance(Tr, 1.0) + got.shape[1] * 2.0 ** -24), (what, "rows sum to 1", sums)
    return float(ratio.max())


def check(got, c, band, verbose=True):
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
            if i >= int(c["n_valid"][b]):
                assert got.logp[b, i] != got.logp[b, i], ("unscored rows are NaN", b, i)
                continue
            post, lp = refs[(b, i)]
            assert SC.same(got.logp[b, i], lp, Tr), (c["name"], band, b, i, got.logp[b, i], lp)
            n = post.shape[0]
            worst = max(worst, check_one(got.post[b, i, :n], post, Tr, (c["name"], "band", band, b, i)))
            if N == 2 and math.isfinite(lp):
                assert np.all(np.abs(got.post[b, i, :n] - 1.0) <= tolerance(Tr, 1.0)), (c["name"], b, i)
    if verbose:
        print("ctc_posterior: %s band %d, %d labellings, worst |error| / tolerance = %.3f" % (c["name"], band, len(refs), worst))


def run_case(fcd, c, device=None):
    """the case at each of its bands (numpy through _host, or torch tensors on `device` through _dev) against the
    restatement; a band wider than a labelling gives what exact mode gives, within the tolerance"""
    kw = {}
    if device is None:
        xin = c["xin"]
        if c["dtype"] == "bf16":
            kw["input_dtype"] = "bfloat16"
        conv = lambda a: a
    else:
        import torch
        if c["dtype"] == "bf16":
            xin = torch.from_numpy(np.ascontiguousarray(c["xin"]).view(np.int16)).to(device).view(torch.bfloat16)
        else:
            xin = torch.from_numpy(np.ascontiguousarray(c["xin"])).to(device)
        if c["xin"].strides[0] < c["xin"].strides[1]:  # time-major on the device too
            xin = xin.transpose(0, 1).contiguous().transpose(0, 1)
        conv = lambda a: None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device)
    by_band = {}
    for band in c["bands"]:
        got = fcd.ctc_posterior_batch_raw(xin, conv(c["labels"]), conv(c["out_len"]), c["collapse"], conv(c["lengths"]),
                                          conv(c["paths"]) if band else None, band, conv(c["n_valid"]), **kw)
        if device is not None:
            assert got.post.device == xin.device and got.logp.device == xin.device
            got = got.cpu()
        check(got, c, band)
        by_band[band] = got
    if 0 in by_band:
        B, n_hyp = c["out_len"].shape
        for band, got in by_band.items():
            for b in range(B):
                Tr = c["T"] if c["lengths"] is None else int(c["lengths"][b])
                for i in range(min(n_hyp, int(c["n_valid"][b]))):
                    n = int(c["out_len"][b, i])
                    if band > n and math.isfinite(by_band[0].logp[b, i]):
                        ex = by_band[0].post[b, i, :n].astype(np.float64)
                        assert np.all(np.abs(got.post[b, i, :n] - ex) <= 2 * tolerance(Tr, ex)), (c["name"], band, b, i)
    return by_band


def edge_batch():
    """-> (x, labels, lens, lengths): the edge rows of include/fcd.h
    0: L = 0   1: T_r = 0, L = 0   2: T_r = 0, L > 0   3: L > T_r   4: label N   5: label 0   6: a NaN posterior
    7: repeats that need more rows than there are   8: an ordinary row   9: len > stride"""
    rng = np.random.default_rng(4)
    x = SC.posteriors(rng, 10, 6, 4)
    labels = np.zeros((10, 8), np.uint8)
    lens = np.zeros(10, np.uint32)
    lengths = np.full(10, 6, np.int64)
    lengths[1] = lengths[2] = 0
    labels[2, :1], lens[2] = [1], 1
    labels[3, :7], lens[3] = [1, 2, 1, 2, 1, 2, 1], 7
    labels[4, :2], lens[4] = [1, 4], 2
    labels[5, :2], lens[5] = [2, 0], 2
    labels[6, :2], lens[6] = [1, 2], 2
    x[6, 3, 0] = np.nan
    labels[7, :4], lens[7] = [3, 3, 3, 3], 4
    labels[8, :3], lens[8] = [1, 1, 3], 3
    labels[9, :], lens[9] = 1, 9
    return x, labels, lens, lengths


def check_edges(post, logp, x, labels, lens, lengths, unwritten):
    """post (10, 8, 3), logp (10,) of edge_batch(); entries the call must not write hold `unwritten`"""
    lp = logp
    assert abs(lp[0] - np.log(x[0, :, 0].astype(np.float64)).sum()) <= 6 * 2.0 ** -24 and lp[1] == 0.0
    assert lp[2] == -math.inf and lp[3] == -math.inf and lp[7] == -math.inf
    assert all(math.isnan(lp[b]) for b in (4, 5, 6, 9))
    for b in range(10):
        n = min(int(lens[b]), 8)
        if b == 8:
            ref, rlp = PR.ctc_posterior(x[8], labels[8, :3])
            assert SC.same(lp[8], rlp, 6)
            check_one(post[8, :3], ref, 6, "edge row 8")
        else:
            assert np.isnan(post[b, :n]).all(), (b, post[b, :n])
        assert (post[b, n:] == unwritten).all(), (b, "entries k >= len", post[b, n:])
