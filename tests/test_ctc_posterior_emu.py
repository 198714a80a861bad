"""CPU-side check of the substitution-posterior kernels (csrc/ctc_posterior.hip, compiled against tests/hipemu's lockstep
wave64 emulation) through ctc_posterior_batch_raw on numpy, against the restatement tests/ctc_posterior_reference.py: the
cases of tests/ctc_posterior_cases.py (all four register tiers, N = 2 / 5 / 9, f16 / bf16, time-major strides, ragged
lengths, both collapse_repeats values, bands 0 / 1 / 4 / 64), every edge row of include/fcd.h, the argument errors at both
layers, the two limits, the results' own ctc_posterior, the single-read function, and a workspace limit that forces
several groups.  The -m gpu twin is tests/test_gpu_ctc_posterior.py."""
import ctypes as C
import math

import numpy as np
import pytest

import ctc_posterior_cases as PC
import ctc_posterior_reference as PR
import ctc_score_cases as SC
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("case", PC.CASES, ids=[c[0] for c in PC.CASES])
def test_against_restatement(fcd, case):
    PC.run_case(fcd, PC.build_case(fcd, case))


def test_edge_rows(fcd):
    x, labels, lens, lengths = PC.edge_batch()
    got = fcd.ctc_posterior_batch_raw(x, labels, lens, lengths=lengths)
    PC.check_edges(got.post[:, 0], got.logp[:, 0], x, labels, lens, lengths, 0.0)  # (_host: entries k >= len are 0)
    # i >= n_valid: NaN logp, and NaN for the labels the row claims to hold
    lab2 = np.stack([labels, labels], 1)
    len2 = np.stack([lens, lens], 1)
    nv = np.ones(10, np.uint32)
    got2 = fcd.ctc_posterior_batch_raw(x, lab2, len2, lengths=lengths, n_valid=nv)
    assert np.array_equal(got2.post[:, 0], got.post[:, 0], equal_nan=True) and np.isnan(got2.logp[:, 1]).all()
    assert np.isnan(got2.post[8, 1, :3]).all() and (got2.post[8, 1, 3:] == 0).all()
    # every row emits (collapse_repeats = 0): read 7 has an alignment, one row per label
    nc = fcd.ctc_posterior_batch_raw(x, labels, lens, False, lengths)
    ref, lp = PR.ctc_posterior(x[7], labels[7, :4], False)
    assert SC.same(nc.logp[7, 0], lp, 6)
    PC.check_one(nc.post[7, 0, :4], ref, 6, "no collapse, read 7")
    # a NaN posterior in a column the labelling does not read: logp stands, the positions that see it are NaN
    xn = x[8:9].copy()
    xn[0, 2, 2] = np.nan
    gn = fcd.ctc_posterior_batch_raw(xn, labels[8:9], lens[8:9])
    ref, lp = PR.ctc_posterior(xn[0], labels[8, :3])
    assert math.isfinite(lp) and SC.same(gn.logp[0, 0], lp, 6)
    PC.check_one(gn.post[0, 0, :3], ref, 6, "NaN in a variant's column")
    # very small posteriors (the row maximum falls by 2^-100 in one step): nothing is lost
    tiny = x[8:9].copy()
    tiny[0, 2, :] *= np.float32(2.0 ** -100)
    tiny[0, 4, :] *= np.float32(2.0 ** -120)
    gt = fcd.ctc_posterior_batch_raw(tiny, labels[8:9], lens[8:9])
    PC.check_one(gt.post[0, 0, :3], PR.ctc_posterior(tiny[0], labels[8, :3])[0], 6, "tiny rows")


def test_argument_errors_and_limits(fcd):
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(6)
    x = SC.posteriors(rng, 2, 10, 5)
    labels = np.ones((2, 10), np.uint8)
    lens = np.array([3, 4], np.uint32)
    with pytest.raises(ValueError):
        fcd.ctc_posterior_batch_raw(x, labels, lens, band=-1)
    with pytest.raises(ValueError):
        fcd.ctc_posterior_batch_raw(x, labels, lens, band=4)  # no paths
    with pytest.raises(TypeError):
        fcd.ctc_posterior_batch_raw(x, labels, lens, band=1.5)
    with pytest.raises(ValueError):
        fcd.ctc_posterior_batch_raw(x, labels[:1], lens)
    with pytest.raises(ValueError):
        fcd.ctc_posterior_batch_raw(x, labels, lens[:1])
    with pytest.raises(ValueError):
        fcd.ctc_posterior_batch_raw(x, labels, lens, paths=np.zeros((2, 9), np.uint32), band=2)
    # the C ABI refuses them itself, before anything is enqueued or written
    h = nat.default_handle()
    path = np.zeros((2, 10), np.uint32)
    po, lp = np.full((2, 10, 4), 77.0, np.float32), np.full(2, 77.0)

    def call(S=1, n_hyp=1, band=0, with_path=True, fn="fcd_ctc_posterior_host", post=True, logp=True):
        b = nat.Batch(x.ctypes.data, 2, 10, S, 5, 50, 5, 0, 1, None)
        y = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, path.ctypes.data if with_path else None, n_hyp, 10)
        out = nat.Posterior(po.ctypes.data if post else None, lp.ctypes.data if logp else None)
        return getattr(h.lib, fn)(h.ptr, C.byref(b), C.byref(y), 1, band, C.byref(out))
    for fn in ("fcd_ctc_posterior_host", "fcd_ctc_posterior_dev"):
        assert call(band=-1, fn=fn) == nat.E_INVALID
        assert call(band=3, with_path=False, fn=fn) == nat.E_INVALID
        assert call(n_hyp=0, fn=fn) == nat.E_INVALID
        assert call(S=4, fn=fn) == nat.E_INVALID
        assert call(post=False, fn=fn) == nat.E_INVALID
        b = nat.Batch(x.ctypes.data, 2, 10, 1, 5, 50, 5, 0, 1, None)
        y = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, None, 1, 10)
        assert getattr(h.lib, fn)(h.ptr, C.byref(b), C.byref(y), 1, 0, None) == nat.E_INVALID
    assert (po == 77).all() and (lp == 77).all()
    assert call(logp=False) == nat.OK and (lp == 77).all() and np.isfinite(po[0, :3]).all()  # (logp is optional)
    assert call() == nat.OK and np.isfinite(lp).all()
    # the limits: unsupported, and the message names the way out
    for T, N, band, msg in ((600, 5, 0, b"use a band"), (600, 5, 127, b"narrower band"), (40, 10, 0, b"8 labels"),
                            (40000, 5, 4, b"smaller stride")):
        b = nat.Batch(None, 0, T, 1, N, T * N, N, 0, 1, None)
        y = nat.Labellings(None, None, None, path.ctypes.data, 1, T)
        out = nat.Posterior(None, None)
        assert h.lib.fcd_ctc_posterior_host(h.ptr, C.byref(b), C.byref(y), 1, band, C.byref(out)) == nat.E_UNSUPPORTED
        assert msg in h.lib.fcd_last_error(h.ptr), h.lib.fcd_last_error(h.ptr)
    b = nat.Batch(None, 0, 600, 1, 5, 3000, 5, 0, 1, None)
    y = nat.Labellings(None, None, None, path.ctypes.data, 1, 600)
    assert h.lib.fcd_ctc_posterior_host(h.ptr, C.byref(b), C.byref(y), 1, 126, C.byref(nat.Posterior(None, None))) == nat.OK
    with pytest.raises(nat.NativeError) as e:
        fcd.ctc_posterior_batch_raw(SC.posteriors(rng, 1, 600, 5), np.ones((1, 600), np.uint8), [5])
    assert e.value.code == nat.E_UNSUPPORTED
    with pytest.raises(nat.NativeError) as e:
        fcd.ctc_posterior_batch_raw(SC.posteriors(rng, 1, 20, 10), np.ones((1, 20), np.uint8), [5])
    assert e.value.code == nat.E_UNSUPPORTED


def test_results_score_themselves(fcd):
    rng = np.random.default_rng(7)
    x = SC.posteriors(rng, 4, 30, 5)
    lengths = np.array([30, 17, 1, 26], np.int64)
    r = fcd.beam_search_batch_raw(x, 5, 0.0, lengths=lengths)
    for band in (0, 4):
        got = r.ctc_posterior(x, lengths=lengths, band=band)
        assert got.post.shape == (4, 1, 30, 4) and got.logp.shape == (4, 1)
        for b in range(4):
            n = int(r.out_len[b])
            ref, lp = PR.ctc_posterior(x[b, :lengths[b]], r.labels[b, :n], True, band, r.path[b, :n] if band else None)
            assert SC.same(got.logp[b, 0], lp, int(lengths[b]))
            PC.check_one(got.post[b, 0, :n], ref, int(lengths[b]), ("BatchResult", band, b))
    conf = got.conf(r.labels)
    assert conf.shape == (4, 1, 30) and conf.dtype == np.float32
    n0 = int(r.out_len[0])
    assert np.array_equal(conf[0, 0, :n0], got.post[0, 0, np.arange(n0), r.labels[0, :n0].astype(int) - 1])
    assert (conf[0, 0, n0:] == 0).all()
    qs = got.qstrings(r.labels, r.out_len)
    lib = fcd._native.load()
    assert qs[0][0] == "".join(chr(lib.fcd_phred(float(q), 1.0, 0.0)) for q in conf[0, 0, :n0])
    assert qs == got.cpu().qstrings(r.labels, r.out_len) and [len(q[0]) for q in qs] == [int(n) for n in r.out_len]
    nb = fcd.beam_search_nbest_batch_raw(x, 3, beam_size=5, lengths=lengths)
    g = nb.ctc_posterior(x, lengths=lengths, band=64)
    assert g.post.shape == (4, 3, 30, 4)
    for b in range(4):
        for i in range(3):
            if i >= int(nb.n_hyp[b]):
                assert math.isnan(g.logp[b, i])
                continue
            n = int(nb.out_len[b, i])
            ref, lp = PR.ctc_posterior(x[b, :lengths[b]], nb.labels[b, i, :n], True, 64, nb.path[b, i, :n])
            PC.check_one(g.post[b, i, :n], ref, int(lengths[b]), ("NBestResult", b, i))
    assert len(g.qstrings(nb.labels, nb.out_len)) == 4
    # CRF results are refused
    xc = np.abs(rng.standard_normal((2, 6, 4, 5))).astype(np.float32)
    init = np.ones((2, 4), np.float32)
    with pytest.raises(ValueError, match="CRF"):
        fcd.crf_beam_search_batch_raw(xc, init, 5, 0.0).ctc_posterior(xc)
    with pytest.raises(ValueError, match="CRF"):
        fcd.crf_beam_search_nbest_batch_raw(xc, init, 2, 5, 0.0).ctc_posterior(xc)


def test_single_read_function(fcd):
    rng = np.random.default_rng(5)
    x = SC.posteriors(rng, 1, 30, 5)[0]
    seq, _ = fcd.beam_search(x, "NACGT", 5)
    post, logp = fcd.ctc_posterior(x, seq, "NACGT")
    ref, lp = PR.ctc_posterior(x, ["NACGT".index(c) for c in seq])
    assert post.shape == (len(seq), 4) and post.dtype == np.float32 and isinstance(logp, float) and SC.same(logp, lp, 30)
    PC.check_one(post, ref, 30, "single read")
    assert abs(logp - fcd.ctc_score(x, seq, "NACGT")) <= SC.tolerance(30)
    empty, lp0 = fcd.ctc_posterior(x, "", "NACGT")
    assert empty.shape == (0, 4) and math.isfinite(lp0)
    none, lpi = fcd.ctc_posterior(x[:2], "ACGT", "NACGT")
    assert lpi == -math.inf and np.isnan(none).all()
    with pytest.raises(ValueError, match="alphabet size"):
        fcd.ctc_posterior(x, seq, "NACG")
    with pytest.raises(ValueError, match="single-character"):
        fcd.ctc_posterior(x, seq, ["N", "AB", "C", "G", "T"])
    with pytest.raises(ValueError, match="not a label"):
        fcd.ctc_posterior(x, "AN", "NACGT")
    with pytest.raises(TypeError):
        fcd.ctc_posterior(x, [1, 2], "NACGT")


def test_workspace_limit_groups(fcd):
    """a workspace limit of one byte: every read is a launch pair of its own, in the same memory; the same values"""
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(8)
    x = SC.posteriors(rng, 6, 40, 5)
    lengths = np.array([40, 17, 40, 1, 33, 40], np.int64)
    h = nat.default_handle()
    r = fcd.beam_search_batch_raw(x, 5, 0.0, lengths=lengths)
    nb = fcd.beam_search_nbest_batch_raw(x[:3], 2, beam_size=5, lengths=lengths[:3])
    for res, xs, ls in ((r, x, lengths), (nb, x[:3], lengths[:3])):
        for band in (0, 4):
            whole = res.ctc_posterior(xs, lengths=ls, band=band)
            h.set_workspace_limit(1)
            try:
                parts = res.ctc_posterior(xs, lengths=ls, band=band)
            finally:
                h.set_workspace_limit(0)
            assert np.array_equal(whole.post, parts.post, equal_nan=True) and np.array_equal(whole.logp, parts.logp, equal_nan=True)
            assert np.isfinite(whole.logp[:, 0]).all()
