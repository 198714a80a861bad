"""CPU-side check of the CTC forced-alignment kernels (csrc/ctc_align.hip, compiled against tests/hipemu's lockstep wave64
emulation) through ctc_align_batch_raw on numpy, against the restatement tests/ctc_align_reference.py: the shape grid of
tests/ctc_score_cases.py (alphabets of 2 .. 12 labels, 9 .. 300 rows, ragged lengths, f16 / bf16 input, time-major strides,
1 .. 5 hypotheses with n_valid, both collapse_repeats values, exact mode and bands 1 / 4 / 64 / 128, windows that live in
registers at 2, 4, 6, 8 states per lane and in LDS), every edge case of include/fcd.h, the argument errors at both layers,
every combination of the C ABI's optional pointers through fcd_ctc_align_host, the workspace cap forcing several launches, the results' own ctc_align, beam_search(qstring=True), and parity with
viterbi_search on its own output.  What is compared and how: tests/ctc_align_cases.py.  The -m gpu twin is
tests/test_gpu_ctc_align.py."""
import ctypes as C
import math

import numpy as np
import pytest

import ctc_align_cases as AC
import ctc_align_reference as A
import ctc_score_cases as SC
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("case", SC.CASES, ids=[c[0] for c in SC.CASES])
def test_against_restatement(fcd, case):
    AC.run_case(fcd, SC.build_case(fcd, case))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("T", [1, 65, 200])
def test_greedy_parity(fcd, T, dtype):
    AC.greedy_parity(fcd, T, dtype)
    if T == 65:
        AC.greedy_parity(fcd, T, dtype, collapse=False)


def test_edge_cases(fcd):
    rng = np.random.default_rng(4)
    x = SC.posteriors(rng, 12, 6, 4)
    labels = np.zeros((12, 8), np.uint8)
    lens = np.zeros(12, np.uint32)
    lengths = np.full(12, 6, np.int64)
    # 0: L = 0            1: T_r = 0, L = 0     2: T_r = 0, L > 0     3: L > T_r
    # 4: label N          5: label 0            6: a NaN posterior    7: repeats that need a blank more than there are rows
    # 8: an infinity      9: a negative value   10: len > stride      11: a NaN posterior, but L > T_r comes first
    lengths[1] = lengths[2] = 0
    labels[2, :1], lens[2] = [1], 1
    labels[3, :7], lens[3] = [1, 2, 1, 2, 1, 2, 1], 7
    labels[4, :2], lens[4] = [1, 4], 2
    labels[5, :2], lens[5] = [2, 0], 2
    labels[6, :2], lens[6] = [1, 2], 2
    x[6, 3, 0] = np.nan
    labels[7, :4], lens[7] = [3, 3, 3, 3], 4
    labels[8, :2], lens[8] = [1, 2], 2
    x[8, 5, 3] = np.inf  # (a column no state of the labelling reads: anywhere in the read counts)
    labels[9, :2], lens[9] = [1, 2], 2
    x[9, 0, 3] = -0.5
    labels[10, :], lens[10] = 1, 9
    labels[11, :7], lens[11] = [1, 2, 1, 2, 1, 2, 1], 7
    x[11, 2, 1] = np.nan
    got = fcd.ctc_align_batch_raw(x, labels, lens, lengths=lengths)
    lp = got.logp[:, 0]
    assert abs(lp[0] - np.log(x[0, :, 0].astype(np.float64)).sum()) <= 6 * 2.0 ** -24
    assert lp[1] == 0.0
    assert lp[2] == -math.inf and lp[3] == -math.inf and lp[7] == -math.inf and lp[11] == -math.inf
    assert all(math.isnan(lp[b]) for b in (4, 5, 6, 8, 9, 10))
    assert (got.count == 0).all() and (got.start == 0).all()  # no read of this batch has an alignment with labels
    for b in range(12):
        if b != 10:
            assert AC.logp_same(lp[b], A.ctc_align(x[b, :lengths[b]], labels[b, :lens[b]])["logp"]), b
    # count = 0 is WRITTEN (the device entry point leaves the other arrays alone): poisoned outputs through the C ABI
    from fast_ctc_decode_amd import _native as nat
    h = nat.default_handle()
    st, ct = np.full((12, 8), 77, np.uint32), np.full((12, 8), 77, np.uint32)
    out = nat.Alignment(st.ctypes.data, ct.ctypes.data, None, None)  # (qual and logp are optional)
    b_ = nat.Batch(x.ctypes.data, 12, 6, 1, 4, 24, 4, 0, 1, lengths.ctypes.data)
    y_ = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, None, 1, 8)
    assert h.lib.fcd_ctc_align_host(h.ptr, C.byref(b_), C.byref(y_), 1, 0, C.byref(out)) == nat.OK
    assert (ct == 0).all()
    # every row emits (collapse_repeats = 0): 4 rows do for read 7, one row per label
    nc = fcd.ctc_align_batch_raw(x, labels, lens, False, lengths)
    assert nc.logp[7, 0] > -math.inf and nc.count[7, 0, :4].tolist() == [1, 1, 1, 1]
    AC.check(nc, x, lengths, labels[:, None], None, lens[:, None], None, False, 0, rows=[0, 1, 2, 3, 7])
    # a band wider than the labelling, path given: the exact alignment
    y = np.array([[1, 2, 3, 0, 0, 0, 0, 0]], np.uint8)
    pth = np.array([[0, 2, 5, 0, 0, 0, 0, 0]], np.uint32)
    one, ex = fcd.ctc_align_batch_raw(x[:1], y, [3], paths=pth, band=64), fcd.ctc_align_batch_raw(x[:1], y, [3])
    assert one.logp[0, 0] == ex.logp[0, 0] and np.array_equal(one.start, ex.start) and np.array_equal(one.count, ex.count)
    AC.check(ex, x[:1], None, y[:, None], None, np.array([[3]]), None, True, 0)
    # very small posteriors (the row maximum falls by 2^-100 in one step), and a zero column: nothing is lost
    tiny = x[:1].copy()
    tiny[0, 2, :] *= np.float32(2.0 ** -100)
    tiny[0, 4, :] *= np.float32(2.0 ** -120)
    tiny[0, 1, 2] = 0.0
    AC.check(fcd.ctc_align_batch_raw(tiny, y, [3]), tiny, None, y[:, None], None, np.array([[3]]), None, True, 0)
    # a band whose window never reaches the last states: no alignment inside it
    far = np.array([[0, 0, 0, 0, 0, 0, 0, 0]], np.uint32)
    xl = SC.posteriors(rng, 1, 40, 4)
    yl = np.tile(np.array([1, 2, 3], np.uint8), 5)[None, :]
    pl = np.arange(15, dtype=np.uint32)[None, :] + 25  # every label late: k(t) = 0 for 25 rows, band 1 ends at state 2
    got = fcd.ctc_align_batch_raw(xl, yl, [15], paths=pl, band=1)
    ref = A.ctc_align(xl[0], yl[0], True, 1, pl[0])
    assert AC.logp_same(got.logp[0, 0], ref["logp"])
    AC.check(got, xl, None, yl[:, None], pl[:, None], np.array([[15]]), None, True, 1)


def test_host_abi_optional_pointers(fcd):
    AC.host_abi_optional_pointers(fcd)


def test_single_read_function(fcd):
    rng = np.random.default_rng(5)
    x = SC.posteriors(rng, 1, 30, 5)[0]
    seq, _ = fcd.beam_search(x, "NACGT", 5)
    spans, quals, logp = fcd.ctc_align(x, seq, "NACGT")
    ref = A.ctc_align(x, ["NACGT".index(c) for c in seq])
    assert spans == list(zip(ref["start"], ref["count"])) and isinstance(logp, float) and AC.logp_same(logp, ref["logp"])
    assert [np.float32(q) for q in quals] == ref["qual"] and all(isinstance(q, float) for q in quals)
    assert fcd.ctc_align(x, "", "NACGT")[:2] == ([], [])
    assert fcd.ctc_align(x[:2], "ACGT", "NACGT") == ([], [], -math.inf)
    with pytest.raises(ValueError, match="alphabet size"):
        fcd.ctc_align(x, seq, "NACG")
    with pytest.raises(ValueError, match="single-character"):
        fcd.ctc_align(x, seq, ["N", "AB", "C", "G", "T"])
    with pytest.raises(ValueError, match="not a label"):
        fcd.ctc_align(x, "AN", "NACGT")
    with pytest.raises(TypeError):
        fcd.ctc_align(x, [1, 2], "NACGT")


def test_argument_errors(fcd):
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(6)
    x = SC.posteriors(rng, 2, 10, 5)
    labels = np.ones((2, 10), np.uint8)
    lens = np.array([3, 4], np.uint32)
    with pytest.raises(ValueError):
        fcd.ctc_align_batch_raw(x, labels, lens, band=-1)
    with pytest.raises(ValueError):
        fcd.ctc_align_batch_raw(x, labels, lens, band=4)  # no paths
    with pytest.raises(TypeError):
        fcd.ctc_align_batch_raw(x, labels, lens, band=1.5)
    with pytest.raises(ValueError):
        fcd.ctc_align_batch_raw(x, labels[:1], lens)
    with pytest.raises(ValueError):
        fcd.ctc_align_batch_raw(x, labels, lens[:1])
    with pytest.raises(ValueError):
        fcd.ctc_align_batch_raw(x, labels, lens, paths=np.zeros((2, 9), np.uint32), band=2)
    # the C ABI refuses them itself, before anything is enqueued or written
    h = nat.default_handle()
    path = np.zeros((2, 10), np.uint32)
    st, ct = np.full((2, 10), 77, np.uint32), np.full((2, 10), 77, np.uint32)
    ql, lp = np.full((2, 10), 77.0, np.float32), np.full(2, 77.0)

    def call(S=1, n_hyp=1, band=0, with_path=True, fn="fcd_ctc_align_host", start=True, count=True):
        b = nat.Batch(x.ctypes.data, 2, 10, S, 5, 50, 5, 0, 1, None)
        y = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, path.ctypes.data if with_path else None, n_hyp, 10)
        out = nat.Alignment(st.ctypes.data if start else None, ct.ctypes.data if count else None, ql.ctypes.data, lp.ctypes.data)
        return getattr(h.lib, fn)(h.ptr, C.byref(b), C.byref(y), 1, band, C.byref(out))
    for fn in ("fcd_ctc_align_host", "fcd_ctc_align_dev"):
        assert call(band=-1, fn=fn) == nat.E_INVALID
        assert call(band=3, with_path=False, fn=fn) == nat.E_INVALID
        assert call(n_hyp=0, fn=fn) == nat.E_INVALID
        assert call(S=4, fn=fn) == nat.E_INVALID
        assert call(start=False, fn=fn) == nat.E_INVALID
        assert call(count=False, fn=fn) == nat.E_INVALID
        b = nat.Batch(x.ctypes.data, 2, 10, 1, 5, 50, 5, 0, 1, None)
        y = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, None, 1, 10)
        assert getattr(h.lib, fn)(h.ptr, C.byref(b), C.byref(y), 1, 0, None) == nat.E_INVALID
    assert (st == 77).all() and (ct == 77).all() and (ql == 77).all() and (lp == 77).all()
    assert h.lib.fcd_debug_set_align_workspace_cap(h.ptr, -1) == nat.E_INVALID
    assert call() == nat.OK and np.isfinite(lp).all() and (ct[0, :3] >= 1).all()
    # a window beyond the LDS: unsupported, and the message names the way out
    T = 12000
    b = nat.Batch(None, 0, T, 1, 5, T * 5, 5, 0, 1, None)
    y = nat.Labellings(None, None, None, None, 1, T)
    out = nat.Alignment(None, None, None, None)
    assert h.lib.fcd_ctc_align_host(h.ptr, C.byref(b), C.byref(y), 1, 0, C.byref(out)) == nat.E_UNSUPPORTED
    assert b"use a band" in h.lib.fcd_last_error(h.ptr)
    y = nat.Labellings(None, None, None, path.ctypes.data, 1, T)
    assert h.lib.fcd_ctc_align_host(h.ptr, C.byref(b), C.byref(y), 1, 64, C.byref(out)) == nat.OK


def test_workspace_cap_groups(fcd):
    """a cap of one byte: every read is a launch of its own -- 6 groups on 6 rows (n_hyp = 1), 3 on 6 (n_hyp = 2)"""
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(8)
    x = SC.posteriors(rng, 6, 40, 5)
    lengths = np.array([40, 17, 40, 1, 33, 40], np.int64)
    h = nat.default_handle()
    r = fcd.beam_search_batch_raw(x, 5, 0.0, lengths=lengths)
    nb = fcd.beam_search_nbest_batch_raw(x[:3], 2, beam_size=5, lengths=lengths[:3])
    for res, xs, ls in ((r, x, lengths), (nb, x[:3], lengths[:3])):
        for band in (0, 4):
            whole = res.ctc_align(xs, lengths=ls, band=band)
            h.set_align_workspace_cap(1)
            try:
                parts = res.ctc_align(xs, lengths=ls, band=band)
            finally:
                h.set_align_workspace_cap(0)
            for name in ("start", "count", "qual", "logp"):
                assert np.array_equal(getattr(whole, name), getattr(parts, name), equal_nan=True), (name, band)
            assert np.isfinite(whole.logp[:, 0]).all()


def test_results_align_themselves(fcd):
    rng = np.random.default_rng(7)
    x = SC.posteriors(rng, 5, 50, 5)
    lengths = np.array([50, 31, 50, 1, 44], np.int64)
    r = fcd.beam_search_batch_raw(x, 5, 0.0, lengths=lengths)
    for band in (0, 4):
        got = r.ctc_align(x, lengths=lengths, band=band)
        assert got.logp.shape == (5, 1) and got.start.shape == (5, 1, 50)
        AC.check(got, x, lengths, r.labels[:, None, :], r.path[:, None, :], r.out_len[:, None], None, True, band)
    nb = fcd.beam_search_nbest_batch_raw(x, 4, beam_size=6, beam_cut_threshold=0.05, lengths=lengths)
    for band in (0, 64):
        got = nb.ctc_align(x, lengths=lengths, band=band)
        assert got.logp.shape == (5, 4)
        AC.check(got, x, lengths, nb.labels, nb.path, nb.out_len, nb.n_hyp, True, band)
    qs = nb.ctc_align(x, lengths=lengths).qstrings(nb.out_len)
    assert len(qs) == 5 and all(len(q) == 4 for q in qs)
    for b in range(5):
        for i in range(4):
            assert len(qs[b][i]) == (int(nb.out_len[b, i]) if i < int(nb.n_hyp[b]) else 0)
    # CRF results are refused
    xc = np.abs(rng.standard_normal((2, 6, 4, 5))).astype(np.float32)
    init = np.ones((2, 4), np.float32)
    with pytest.raises(ValueError, match="CRF"):
        fcd.crf_beam_search_batch_raw(xc, init, 5, 0.0).ctc_align(xc)
    with pytest.raises(ValueError, match="CRF"):
        fcd.crf_beam_search_nbest_batch_raw(xc, init, 2, 5, 0.0).ctc_align(xc)


def test_beam_search_qstring(fcd):
    rng = np.random.default_rng(9)
    x = SC.posteriors(rng, 1, 60, 5)[0]
    plain = fcd.beam_search(x, "NACGT", 5, 0.0)
    assert plain == fcd.beam_search(x, "NACGT", 5, 0.0, True)  # every existing call: unchanged
    seq, path = fcd.beam_search(x, "NACGT", 5, 0.0, qstring=True)
    n = len(plain[0])
    assert n > 0 and path == plain[1] and seq[:n] == plain[0] and len(seq) == 2 * n
    _, quals, _ = fcd.ctc_align(x, plain[0], "NACGT")
    lib = fcd._native.load()
    assert seq[n:] == "".join(chr(lib.fcd_phred(q, 1.0, 0.0)) for q in quals)
    biased = fcd.beam_search(x, "NACGT", 5, 0.0, qstring=True, qscale=2.0, qbias=1.5)[0]
    assert biased[:n] == plain[0] and biased[n:] == "".join(chr(lib.fcd_phred(q, 2.0, 1.5)) for q in quals)
    with pytest.raises(TypeError):
        fcd.beam_search(x, "NACGT", 5, 0.0, True, True)  # the new arguments are keyword-only
    fcd.set_coalescing(8)
    try:
        assert fcd.beam_search(x, "NACGT", 5, 0.0, qstring=True) == (seq, path)
        assert fcd.beam_search(x, "NACGT", 5, 0.0) == plain
    finally:
        fcd.set_coalescing(0)
