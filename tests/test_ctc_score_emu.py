"""CPU-side check of the CTC forward scoring kernels (csrc/ctc_score.hip, compiled against tests/hipemu's lockstep
wave64 emulation) through ctc_score_batch_raw on numpy, against the float64 restatement tests/ctc_score_reference.py:
alphabets of 2 .. 12 labels, 1 .. 300 rows, ragged lengths, f16 / bf16 input, time-major strides, 1 .. 5 hypotheses
with n_valid, both collapse_repeats values, exact mode and bands 1 / 4 / 64 / 128, windows that live in registers
(2, 4, 6, 8 states per lane) and in LDS, every edge case of include/fcd.h, the argument errors, and
BatchResult.ctc_score / NBestResult.ctc_score fed straight from a search.  Tolerance and input condition:
tests/ctc_score_cases.py.  The -m gpu twin is tests/test_gpu_ctc_score.py."""
import ctypes as C
import math

import numpy as np
import pytest

import ctc_score_cases as SC
import ctc_score_reference as R
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("case", SC.CASES, ids=[c[0] for c in SC.CASES])
def test_against_restatement(fcd, case):
    SC.run_case(fcd, SC.build_case(fcd, case), verbose=True)


def test_single_row_and_single_label_alphabet(fcd):
    rng = np.random.default_rng(3)
    for N in (2, 3):
        x = SC.posteriors(rng, 4, 1, N)
        labels = np.array([[0], [1], [1], [N - 1]], np.uint8)
        lens = np.array([0, 1, 1, 1], np.uint32)
        got = fcd.ctc_score_batch_raw(x, labels, lens)
        for b in range(4):
            assert SC.same(got[b, 0], R.ctc_logp(x[b], labels[b, :lens[b]]), 1)


def test_edge_cases(fcd):
    rng = np.random.default_rng(4)
    x = SC.posteriors(rng, 8, 6, 4)
    labels = np.zeros((8, 8), np.uint8)
    lens = np.zeros(8, np.uint32)
    lengths = np.full(8, 6, np.int64)
    # 0: L = 0            1: T_r = 0, L = 0     2: T_r = 0, L > 0     3: L > T_r
    # 4: label N          5: label 0            6: a NaN posterior    7: repeats that need a blank more than there are rows
    lengths[1] = lengths[2] = 0
    labels[2, :1], lens[2] = [1], 1
    labels[3, :7], lens[3] = [1, 2, 1, 2, 1, 2, 1], 7
    labels[4, :2], lens[4] = [1, 4], 2
    labels[5, :2], lens[5] = [2, 0], 2
    labels[6, :2], lens[6] = [1, 2], 2
    x[6, 3, 0] = np.nan
    labels[7, :4], lens[7] = [3, 3, 3, 3], 4
    got = fcd.ctc_score_batch_raw(x, labels, lens, lengths=lengths)[:, 0]
    assert abs(got[0] - np.log(x[0, :, 0].astype(np.float64)).sum()) <= SC.tolerance(6)
    assert got[1] == 0.0
    assert got[2] == -math.inf and got[3] == -math.inf and got[7] == -math.inf
    assert math.isnan(got[4]) and math.isnan(got[5]) and math.isnan(got[6])
    for b in range(8):
        assert SC.same(got[b], R.ctc_logp(x[b, :lengths[b]], labels[b, :lens[b]]), 6), b
    assert fcd.ctc_score_batch_raw(x, labels, lens, False, lengths)[7, 0] > -math.inf  # every row emits: 4 rows do
    # posteriors outside [0, 1], infinities, negative values: the call terminates and writes something
    bad = x.copy()
    bad[0, 2, :] = [np.inf, -1.0, 7.0, -np.inf]
    bad[3, 1, 1] = 1e30
    out = fcd.ctc_score_batch_raw(bad, labels, lens, lengths=lengths)
    assert out.shape == (8, 1)
    # band wider than the labelling, path given: the exact value
    y = np.array([[1, 2, 3, 0, 0, 0, 0, 0]], np.uint8)
    pth = np.array([[0, 2, 5, 0, 0, 0, 0, 0]], np.uint32)
    one = fcd.ctc_score_batch_raw(x[:1], y, [3], paths=pth, band=64)[0, 0]
    assert SC.same(one, R.ctc_logp(x[0], [1, 2, 3]), 6)
    # very small posteriors (the row maximum falls by 2^-100 in one step): nothing is lost
    tiny = x[:1].copy()
    tiny[0, 2, :] *= np.float32(2.0 ** -100)
    tiny[0, 4, :] *= np.float32(2.0 ** -120)
    assert SC.same(fcd.ctc_score_batch_raw(tiny, y, [3])[0, 0], R.ctc_logp(tiny[0], [1, 2, 3]), 6)


def test_single_read_function(fcd):
    rng = np.random.default_rng(5)
    x = SC.posteriors(rng, 1, 30, 5)[0]
    seq, _ = fcd.beam_search(x, "NACGT", 5)
    v = fcd.ctc_score(x, seq, "NACGT")
    assert isinstance(v, float)
    assert SC.same(v, R.ctc_logp(x, ["NACGT".index(c) for c in seq]), 30)
    assert SC.same(fcd.ctc_score(x, "", "NACGT"), R.ctc_logp(x, []), 30)
    assert fcd.ctc_score(x, seq, "NACGT") >= fcd.ctc_score(x, seq[:-1] + ("A" if seq[-1] != "A" else "C"), "NACGT") - 50
    with pytest.raises(ValueError, match="alphabet size"):
        fcd.ctc_score(x, seq, "NACG")
    with pytest.raises(ValueError, match="single-character"):
        fcd.ctc_score(x, seq, ["N", "AB", "C", "G", "T"])
    with pytest.raises(ValueError, match="not a label"):
        fcd.ctc_score(x, "AXC", "NACGT")
    with pytest.raises(ValueError, match="not a label"):
        fcd.ctc_score(x, "AN", "NACGT")  # the blank is no label
    with pytest.raises(TypeError):
        fcd.ctc_score(x.astype(np.float64), seq, "NACGT")
    with pytest.raises(TypeError):
        fcd.ctc_score(x, [1, 2], "NACGT")


def test_argument_errors(fcd):
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(6)
    x = SC.posteriors(rng, 2, 10, 5)
    labels = np.ones((2, 10), np.uint8)
    lens = np.array([3, 4], np.uint32)
    with pytest.raises(ValueError):
        fcd.ctc_score_batch_raw(x, labels, lens, band=-1)
    with pytest.raises(ValueError):
        fcd.ctc_score_batch_raw(x, labels, lens, band=4)  # no paths
    with pytest.raises(TypeError):
        fcd.ctc_score_batch_raw(x, labels, lens, band=1.5)
    with pytest.raises(ValueError):
        fcd.ctc_score_batch_raw(x, labels[:1], lens)
    with pytest.raises(ValueError):
        fcd.ctc_score_batch_raw(x, labels, lens[:1])
    with pytest.raises(ValueError):
        fcd.ctc_score_batch_raw(x, labels, lens, paths=np.zeros((2, 9), np.uint32), band=2)
    # the C ABI refuses them itself, before anything is enqueued
    h = nat.default_handle()
    out = np.full(2, 123.0)
    path = np.zeros((2, 10), np.uint32)

    def call(S=1, n_hyp=1, band=0, with_path=True, fn="fcd_ctc_score_host"):
        b = nat.Batch(x.ctypes.data, 2, 10, S, 5, 50, 5, 0, 1, None)
        y = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, path.ctypes.data if with_path else None, n_hyp, 10)
        return getattr(h.lib, fn)(h.ptr, C.byref(b), C.byref(y), 1, band, out.ctypes.data)
    for fn in ("fcd_ctc_score_host", "fcd_ctc_score_dev"):
        assert call(band=-1, fn=fn) == nat.E_INVALID
        assert call(band=3, with_path=False, fn=fn) == nat.E_INVALID
        assert call(n_hyp=0, fn=fn) == nat.E_INVALID
        assert call(S=4, fn=fn) == nat.E_INVALID
    assert (out == 123.0).all()
    assert call() == nat.OK and np.isfinite(out).all()
    # a window beyond the LDS: unsupported, and the message names the way out
    T = 12000
    b = nat.Batch(None, 0, T, 1, 5, T * 5, 5, 0, 1, None)
    y = nat.Labellings(None, None, None, None, 1, T)
    assert h.lib.fcd_ctc_score_host(h.ptr, C.byref(b), C.byref(y), 1, 0, None) == nat.E_UNSUPPORTED
    assert b"use a band" in h.lib.fcd_last_error(h.ptr)
    y = nat.Labellings(None, None, None, path.ctypes.data, 1, T)
    assert h.lib.fcd_ctc_score_host(h.ptr, C.byref(b), C.byref(y), 1, 64, None) == nat.OK


def test_results_score_themselves(fcd):
    rng = np.random.default_rng(7)
    x = SC.posteriors(rng, 5, 50, 5)
    lengths = np.array([50, 31, 50, 1, 44], np.int64)
    r = fcd.beam_search_batch_raw(x, 5, 0.0, lengths=lengths)
    for band in (0, 4):
        got = r.ctc_score(x, lengths=lengths, band=band)
        assert got.shape == (5, 1)
        SC.check(got, x, lengths, r.labels[:, None, :], r.path[:, None, :], r.out_len[:, None], None, True, band)
    nb = fcd.beam_search_nbest_batch_raw(x, 4, beam_size=6, beam_cut_threshold=0.05, lengths=lengths)
    for band in (0, 64):
        got = nb.ctc_score(x, lengths=lengths, band=band)
        assert got.shape == (5, 4)
        SC.check(got, x, lengths, nb.labels, nb.path, nb.out_len, nb.n_hyp, True, band)
    # hypothesis 0 of the n-best call is the plain call's result, and so is its score
    assert np.array_equal(nb.ctc_score(x, lengths=lengths)[:, 0] > -np.inf, np.ones(5, bool))
    # the exact scores of distinct labellings of one read sum to at most 1
    assert (np.exp(np.nan_to_num(nb.ctc_score(x, lengths=lengths), nan=-np.inf)).sum(1) <= 1.0 + 1e-5).all()
    # CRF results are refused
    xc = np.abs(rng.standard_normal((2, 6, 4, 5))).astype(np.float32)
    init = np.ones((2, 4), np.float32)
    rc = fcd.crf_beam_search_batch_raw(xc, init, 5, 0.0)
    with pytest.raises(ValueError, match="CRF"):
        rc.ctc_score(xc)
    nc = fcd.crf_beam_search_nbest_batch_raw(xc, init, 2, 5, 0.0)
    with pytest.raises(ValueError, match="CRF"):
        nc.ctc_score(xc)
