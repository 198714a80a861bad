"""CPU-side check of the CRF substitution-posterior kernels (csrc/crf_posterior.hip, compiled against tests/hipemu's
lockstep wave64 emulation) through crf_posterior_batch_raw on numpy, against the restatement
tests/crf_posterior_reference.py: the cases of tests/crf_posterior_cases.py (every K at the exact windows of 64 .. 512
states, histories of 1 / 2 / 3 / 5 labels, the one-row table S = 1, N = 3 / 5 / 9, both staging regimes, f16 / bf16,
time-major strides, ragged lengths, n_hyp = 3 with n_valid, bands 1 / 4 / 64), chains cut by the end of the labelling, a
path that pushes the band's window against both cuts, variants heavier than the labelling by more than 2^130, every edge row of include/fcd.h, a row scaled by 2^-100, the argument errors and limits at both
layers, the results' own crf_posterior, the single-read function, and a workspace limit that forces several groups.
The -m gpu twin is tests/test_gpu_crf_posterior.py."""
import ctypes as C
import math

import numpy as np
import pytest

import crf_lattice_cases as CC
import crf_lattice_reference as R
import crf_posterior_cases as PC
import crf_posterior_reference as PR
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("case", PC.CASES, ids=[c[0] for c in PC.CASES])
def test_against_restatement(fcd, case):
    c = PC.build_case(case)
    PC.run_case(fcd, c)
    if c["name"].startswith("m1_s4n5"):  # (the first maximum of a random init row: a trajectory that does not start at 0)
        assert any(R.trajectory(c["init"][b], [], 4, 5)[0] != 0 for b in range(c["B"]))


@pytest.mark.parametrize("S,N", [(4, 5), (16, 5), (64, 5), (1024, 5), (8, 3), (8, 9)])
def test_chains_cut_by_the_end(fcd, S, N):
    PC.chains_cut_by_the_end(fcd, S, N)


def test_single_state_model(fcd):
    PC.single_state_model(fcd)


@pytest.mark.parametrize("band", [1, 4])
def test_band_against_both_cuts(fcd, band):
    PC.band_against_both_cuts(fcd, band)


def test_heavy_variants(fcd):
    PC.heavy_variants(fcd)


def test_edge_rows(fcd):
    x, init, labels, lens, lengths = PC.edge_batch()
    got = fcd.crf_posterior_batch_raw(x, init, labels, lens, lengths=lengths)
    PC.check_edges(got.post[:, 0], got.logp[:, 0], x, init, labels, lens, lengths, 0.0)  # (_host: entries k >= len are 0)
    assert np.array_equal(got.logp, fcd.crf_score_batch_raw(x, init, labels, lens, lengths=lengths), equal_nan=True)
    # i >= n_valid: NaN logp, and NaN for the labels the row claims to hold
    lab2, len2 = np.stack([labels, labels], 1), np.stack([lens, lens], 1)
    got2 = fcd.crf_posterior_batch_raw(x, init, lab2, len2, lengths=lengths, n_valid=np.ones(12, np.uint32))
    assert np.array_equal(got2.post[:, 0], got.post[:, 0], equal_nan=True) and np.isnan(got2.logp[:, 1]).all()
    assert np.isnan(got2.post[8, 1, :3]).all() and (got2.post[8, 1, 3:] == 0).all()
    # very small posteriors (the row maximum falls by 2^-100 in one step), and a zero column: nothing is lost
    tiny = x[8:9].copy()
    tiny[0, 2] *= np.float32(2.0 ** -100)
    tiny[0, 4] *= np.float32(2.0 ** -120)
    tiny[0, 1, :, 2] = 0.0
    gt = fcd.crf_posterior_batch_raw(tiny, init[8:9], labels[8:9], lens[8:9])
    ref, lp = PR.crf_posterior(tiny[0], init[8], labels[8, :3])
    assert math.isfinite(lp) and abs(gt.logp[0, 0] - lp) <= CC.tolerance(6)
    PC.check_one(gt.post[0, 0, :3], ref, 6, "tiny rows")
    # a band whose window never reaches the last state: no alignment inside it, every position NaN
    xl = CC.posteriors(np.random.default_rng(5), 1, 40, 4, 5)
    yl = np.tile(np.array([1, 2, 3], np.uint8), 5)[None, :]
    gl = fcd.crf_posterior_batch_raw(xl, init[:1], yl, [15], paths=np.zeros((1, 15), np.uint32), band=1)
    assert gl.logp[0, 0] == -math.inf and np.isnan(gl.post).all()


def test_argument_errors_and_limits(fcd):
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(6)
    x = CC.posteriors(rng, 2, 10, 4, 5)
    init = np.ones((2, 4), np.float32)
    labels = np.ones((2, 10), np.uint8)
    lens = np.array([3, 4], np.uint32)
    f = fcd.crf_posterior_batch_raw
    with pytest.raises(ValueError):
        f(x, init, labels, lens, band=-1)
    with pytest.raises(ValueError):
        f(x, init, labels, lens, band=4)  # no paths
    with pytest.raises(TypeError):
        f(x, init, labels, lens, band=1.5)
    with pytest.raises(ValueError):
        f(x, init, labels[:1], lens)
    with pytest.raises(ValueError):
        f(x, init, labels, lens[:1])
    with pytest.raises(ValueError):
        f(x, init[:1], labels, lens)
    with pytest.raises(TypeError):
        f(x[:, :, 0], init, labels, lens)  # rank 3: not a CRF batch
    with pytest.raises(ValueError):
        f(x, init, labels, lens, paths=np.zeros((2, 9), np.uint32), band=2)
    # the C ABI refuses them itself, before anything is enqueued or written
    h = nat.default_handle()
    path = np.zeros((2, 10), np.uint32)
    po, lp = np.full((2, 10, 4), 77.0, np.float32), np.full(2, 77.0)

    def call(fn, S=4, n_hyp=1, band=0, with_path=True, post=True, logp=True, with_init=True, n_init=4, out=True):
        b = nat.Batch(x.ctypes.data, 2, 10, S, 5, 200, 20, 5, 1, None)
        y = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, path.ctypes.data if with_path else None, n_hyp, 10)
        o = nat.Posterior(po.ctypes.data if post else None, lp.ctypes.data if logp else None)
        return getattr(h.lib, fn)(h.ptr, C.byref(b), init.ctypes.data if with_init else None, n_init, 4, C.byref(y), band,
                                  C.byref(o) if out else None)
    for fn in ("fcd_crf_posterior_host", "fcd_crf_posterior_dev"):
        assert call(fn, band=-1) == nat.E_INVALID
        assert call(fn, band=3, with_path=False) == nat.E_INVALID
        assert call(fn, n_hyp=0) == nat.E_INVALID
        assert call(fn, S=0) == nat.E_INVALID
        assert call(fn, with_init=False) == nat.E_INVALID
        assert call(fn, n_init=0) == nat.E_INVALID
        assert call(fn, out=False) == nat.E_INVALID
        assert call(fn, post=False) == nat.E_INVALID
    assert (po == 77).all() and (lp == 77).all()
    assert call("fcd_crf_posterior_host", logp=False) == nat.OK and (lp == 77).all() and np.isfinite(po[0, :3]).all()
    assert call("fcd_crf_posterior_host") == nat.OK and np.isfinite(lp).all()
    # the limits: unsupported, and the message names the way out
    #   (T, S, N, band): S = 5 at N = 4 is no power; 10 labels; 513 states; 193 states at m = 3 and at m = 5; 257 states
    #   at eight labels; m = 7 at N = 5
    for T, S, N, band, msg in ((40, 5, 4, 0, b"power of N - 1"), (40, 9, 10, 0, b"8 labels"), (512, 4, 5, 0, b"use a band"),
                               (192, 64, 5, 0, b"band of at most 95"), (600, 1024, 5, 96, b"band of at most 95"),
                               (600, 8, 9, 128, b"band of at most 127"),
                               (40, 16384, 5, 4, b"more labels than the kernels carry"), (40, 6, 3, 0, b"power of N - 1")):
        b = nat.Batch(None, 0, T, S, N, T * S * N, S * N, N, 1, None)
        y = nat.Labellings(None, None, None, path.ctypes.data, 1, T)
        out = nat.Posterior(None, None)
        assert h.lib.fcd_crf_posterior_host(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(y), band, C.byref(out)) == nat.E_UNSUPPORTED
        assert msg in h.lib.fcd_last_error(h.ptr), h.lib.fcd_last_error(h.ptr)
    for T, S, N, band in ((511, 4, 5, 0), (600, 16, 5, 255), (191, 64, 5, 0), (600, 4096, 5, 95), (600, 8, 3, 255),
                          (600, 8, 9, 127), (255, 1, 9, 0)):
        b = nat.Batch(None, 0, T, S, N, T * S * N, S * N, N, 1, None)
        y = nat.Labellings(None, None, None, path.ctypes.data, 1, T)
        assert h.lib.fcd_crf_posterior_host(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(y), band,
                                            C.byref(nat.Posterior(None, None))) == nat.OK, (T, S, N, band)
    with pytest.raises(nat.NativeError) as e:
        f(CC.posteriors(rng, 1, 12, 5, 4), np.ones((1, 5), np.float32), np.ones((1, 12), np.uint8), [5])
    assert e.value.code == nat.E_UNSUPPORTED and "power of N - 1" in str(e.value)
    assert math.isfinite(fcd.crf_score_batch_raw(CC.posteriors(rng, 1, 12, 5, 4), np.ones((1, 5), np.float32),
                                                 np.ones((1, 12), np.uint8), [5])[0, 0])  # (crf_score holds the shape)


def test_results_give_their_posteriors(fcd):
    rng = np.random.default_rng(7)
    x = CC.posteriors(rng, 4, 40, 4, 5)
    init = rng.random((4, 4)).astype(np.float32)
    lengths = np.array([40, 23, 1, 36], np.int64)
    r = fcd.crf_beam_search_batch_raw(x, init, 5, 0.0, lengths=lengths)
    for band in (0, 4):
        got = r.crf_posterior(x, init, lengths=lengths, band=band)
        assert got.post.shape == (4, 1, 40, 4) and got.logp.shape == (4, 1)
        assert np.array_equal(got.logp, r.crf_score(x, init, lengths=lengths, band=band))
        for b in range(4):
            n = int(r.out_len[b])
            ref, lp = PR.crf_posterior(x[b, :lengths[b]], init[b], r.labels[b, :n], band, r.path[b, :n] if band else None)
            PC.check_one(got.post[b, 0, :n], ref, int(lengths[b]), ("BatchResult", band, b))
    conf = got.conf(r.labels)
    n0 = int(r.out_len[0])
    assert conf.shape == (4, 1, 40) and np.array_equal(conf[0, 0, :n0], got.post[0, 0, np.arange(n0), r.labels[0, :n0].astype(int) - 1])
    assert [len(q[0]) for q in got.qstrings(r.labels, r.out_len)] == [int(n) for n in r.out_len]
    nb = fcd.crf_beam_search_nbest_batch_raw(x, init, 3, beam_size=5, lengths=lengths)
    g = nb.crf_posterior(x, init, lengths=lengths, band=64)
    assert g.post.shape == (4, 3, 40, 4)
    for b in range(4):
        for i in range(3):
            if i >= int(nb.n_hyp[b]):
                assert math.isnan(g.logp[b, i])
                continue
            n = int(nb.out_len[b, i])
            ref, lp = PR.crf_posterior(x[b, :lengths[b]], init[b], nb.labels[b, i, :n], 64, nb.path[b, i, :n])
            assert abs(g.logp[b, i] - lp) <= CC.tolerance(int(lengths[b]))
            PC.check_one(g.post[b, i, :n], ref, int(lengths[b]), ("NBestResult", b, i))
    # plain CTC results are refused, and ctc_posterior keeps refusing CRF results
    xp = CC.posteriors(rng, 2, 6, 1, 5)[:, :, 0]
    with pytest.raises(ValueError, match="CRF"):
        fcd.beam_search_batch_raw(xp, 5, 0.0).crf_posterior(xp, init[:2])
    with pytest.raises(ValueError, match="CRF"):
        fcd.beam_search_nbest_batch_raw(xp, 2, 5, 0.0).crf_posterior(xp, init[:2])
    with pytest.raises(ValueError, match="CRF"):
        r.ctc_posterior(x)
    with pytest.raises(ValueError, match="CRF"):
        nb.ctc_posterior(x)


def test_single_read_function(fcd):
    rng = np.random.default_rng(5)
    x = CC.posteriors(rng, 1, 30, 4, 5)[0]
    init = rng.random(4).astype(np.float32)
    seq, _ = fcd.crf_beam_search(x, init, "NACGT", 5)
    post, logp = fcd.crf_posterior(x, init, seq, "NACGT")
    ref, lp = PR.crf_posterior(x, init, ["NACGT".index(c) for c in seq])
    assert post.shape == (len(seq), 4) and post.dtype == np.float32 and isinstance(logp, float)
    assert logp == fcd.crf_score(x, init, seq, "NACGT") and abs(logp - lp) <= CC.tolerance(30)
    PC.check_one(post, ref, 30, "single read")
    empty, lp0 = fcd.crf_posterior(x, init, "", "NACGT")
    assert empty.shape == (0, 4) and math.isfinite(lp0)
    none, lpi = fcd.crf_posterior(x[:2], init, "ACGT", "NACGT")
    assert lpi == -math.inf and np.isnan(none).all()
    with pytest.raises(ValueError, match="alphabet size"):
        fcd.crf_posterior(x, init, seq, "NACG")
    with pytest.raises(ValueError, match="not a label"):
        fcd.crf_posterior(x, init, "AN", "NACGT")
    with pytest.raises(TypeError):
        fcd.crf_posterior(x, init, [1, 2], "NACGT")


def test_workspace_limit_groups(fcd):
    PC.workspace_limit_groups(fcd)
