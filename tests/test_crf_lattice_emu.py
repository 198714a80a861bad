"""CPU-side check of the CRF lattice kernels (csrc/crf_lattice.hip, compiled against tests/hipemu's lockstep wave64
emulation) through crf_score_batch_raw / crf_align_batch_raw on numpy, against the restatement
tests/crf_lattice_reference.py: the grid of tests/crf_lattice_cases.py (S of 1 .. 1024, alphabets of 2 .. 5, 1 .. 1100 rows,
ragged lengths, f16 / bf16 input, time-major strides, 1 .. 5 hypotheses with n_valid, exact mode and bands 1 .. 128, every
K, both staging regimes, the ring wrapped in every K), parity with crf_greedy_search on its own output, every edge case of
include/fcd.h, the argument errors at both layers, every combination of the C ABI's optional pointers
through fcd_crf_align_host, the workspace cap forcing several launches, the results' own methods
and crf_beam_search(qstring=True).  The -m gpu twin is tests/test_gpu_crf_lattice.py."""
import ctypes as C
import math

import numpy as np
import pytest

import crf_lattice_cases as CC
import crf_lattice_reference as R
from ctc_align_cases import host_abi_optional_pointers, logp_same
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("case", CC.CASES, ids=[c[0] for c in CC.CASES])
def test_against_restatement(fcd, case):
    CC.run_case(fcd, CC.build_case(case))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("T", [1, 65, 200])
def test_greedy_parity(fcd, T, dtype):
    CC.greedy_parity(fcd, T, dtype)


def test_edge_cases(fcd):
    rng = np.random.default_rng(4)
    B, T, S, N = 12, 6, 4, 5
    x = CC.posteriors(rng, B, T, S, N)
    init = np.tile(np.array([0.1, 0.7, 0.7, 0.2], np.float32), (B, 1))
    labels = np.zeros((B, 8), np.uint8)
    lens = np.zeros(B, np.uint32)
    lengths = np.full(B, 6, np.int64)
    # 0: L = 0            1: T_r = 0, L = 0     2: T_r = 0, L > 0      3: L > T_r
    # 4: label N          5: label 0            6: a NaN that enters   7: L = T_r
    # 8: an infinity      9: a negative value   10: len > stride       11: a NaN, but L > T_r comes first
    lengths[1] = lengths[2] = 0
    labels[2, :1], lens[2] = [1], 1
    labels[3, :7], lens[3] = [1, 2, 1, 2, 1, 2, 1], 7
    labels[4, :2], lens[4] = [1, 5], 2
    labels[5, :2], lens[5] = [2, 0], 2
    labels[6, :2], lens[6] = [3, 1], 2  # sigma = 1, 2, 0
    x[6, 3, 2, 0] = np.nan
    labels[7, :6], lens[7] = [1, 2, 3, 4, 1, 2], 6
    labels[8, :2], lens[8] = [3, 1], 2
    x[8, 0, 1, 3] = np.inf
    labels[9, :2], lens[9] = [3, 1], 2
    x[9, 1, 1, 0] = -0.5
    labels[10, :], lens[10] = 1, 9
    labels[11, :7], lens[11] = [1, 2, 1, 2, 1, 2, 1], 7
    x[11, 2, 1, 0] = np.nan
    got = fcd.crf_align_batch_raw(x, init, labels, lens, lengths=lengths)
    sc = fcd.crf_score_batch_raw(x, init, labels, lens, lengths=lengths)
    lp = got.logp[:, 0]
    assert abs(lp[0] - np.log(x[0, :, 1, 0].astype(np.float64)).sum()) <= 6 * 2.0 ** -24
    assert abs(sc[0, 0] - lp[0]) <= 6 * 2.0 ** -24
    assert lp[1] == 0.0 and sc[1, 0] == 0.0
    assert lp[2] == -math.inf and lp[3] == -math.inf and lp[11] == -math.inf
    assert sc[2, 0] == -math.inf and sc[3, 0] == -math.inf and sc[11, 0] == -math.inf
    assert all(math.isnan(lp[b]) for b in (4, 5, 6, 8, 9, 10)) and all(math.isnan(sc[b, 0]) for b in (4, 5, 6, 10))
    assert got.start[7, 0, :6].tolist() == list(range(6)) and (got.count[7, 0, :6] == 1).all()
    assert (np.delete(got.count, 7, 0) == 0).all() and (np.delete(got.start, 7, 0) == 0).all()
    for b in range(B):
        if b != 10:
            ref = R.crf_align(x[b, :lengths[b]], init[b], labels[b, :lens[b]])
            assert logp_same(lp[b], ref["logp"]), b
            if b not in (8, 9):  # (the score of an infinite or negative posterior is "some value": include/fcd.h)
                want = R.crf_score(x[b, :lengths[b]], init[b], labels[b, :lens[b]])
                assert logp_same(sc[b, 0], want) or abs(sc[b, 0] - want) <= CC.tolerance(6), b
    # a NaN the window never reads changes nothing: another state's row, and state 0's stay past row T - 1 - L
    other = x[6:7].copy()
    other[0, 3, 2, 0] = x[0, 3, 2, 0]
    clean = fcd.crf_align_batch_raw(other, init[:1], labels[6:7], lens[6:7])
    other[0, :, 3, :] = np.nan
    other[0, 5, 1, 0] = np.nan
    again = fcd.crf_align_batch_raw(other, init[:1], labels[6:7], lens[6:7])
    assert math.isfinite(clean.logp[0, 0]) and clean.logp[0, 0] == again.logp[0, 0] and np.array_equal(clean.start, again.start)
    assert fcd.crf_score_batch_raw(other, init[:1], labels[6:7], lens[6:7])[0, 0] == \
        fcd.crf_score_batch_raw(x[:1] * 0 + np.nan_to_num(other), init[:1], labels[6:7], lens[6:7])[0, 0]
    # count = 0 is WRITTEN (the device entry point leaves the other arrays alone): poisoned outputs through the C ABI
    from fast_ctc_decode_amd import _native as nat
    h = nat.default_handle()
    st, ct = np.full((B, 8), 77, np.uint32), np.full((B, 8), 77, np.uint32)
    out = nat.Alignment(st.ctypes.data, ct.ctypes.data, None, None)  # (qual and logp are optional)
    b_ = nat.Batch(x.ctypes.data, B, T, S, N, T * S * N, S * N, N, 1, lengths.ctypes.data)
    y_ = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, None, 1, 8)
    assert h.lib.fcd_crf_align_host(h.ptr, C.byref(b_), init.ctypes.data, 4, 4, C.byref(y_), 0, C.byref(out)) == nat.OK
    assert (np.delete(ct, 7, 0) == 0).all() and (ct[7, :6] == 1).all() and (ct[7, 6:] == 0).all()
    # a state outside the table (S = 5, N = 4): a dead end, except as the state entered at the last row
    x5 = CC.posteriors(rng, 1, 3, 5, 4)
    i6 = np.array([[0, 0, 0, 1, 0]], np.float32)
    y5 = np.array([[3, 1, 0]], np.uint8)
    a1, a2 = fcd.crf_align_batch_raw(x5, i6, y5, [1]), fcd.crf_align_batch_raw(x5, i6, y5, [2])
    assert a1.start[0, 0, 0] == 2 and math.isfinite(a1.logp[0, 0]) and a2.logp[0, 0] == -math.inf and a2.count[0, 0, 0] == 0
    assert fcd.crf_score_batch_raw(x5, i6, y5, [2])[0, 0] == -math.inf
    CC.check(a1, fcd.crf_score_batch_raw(x5, i6, y5, [1]), x5, i6, None, y5[:, None], None, np.array([[1]]), None, 0)
    # a band wider than the labelling, path given: the exact alignment
    y = np.array([[1, 2, 3, 0, 0, 0]], np.uint8)
    pth = np.array([[0, 2, 5, 0, 0, 0]], np.uint32)
    one, ex = fcd.crf_align_batch_raw(x[:1], init[:1], y, [3], paths=pth, band=64), fcd.crf_align_batch_raw(x[:1], init[:1], y, [3])
    assert one.logp[0, 0] == ex.logp[0, 0] and np.array_equal(one.start, ex.start) and np.array_equal(one.count, ex.count)
    # very small posteriors (the row maximum falls by 2^-100 in one step), and a zero column: nothing is lost
    tiny = x[:1].copy()
    tiny[0, 2] *= np.float32(2.0 ** -100)
    tiny[0, 4] *= np.float32(2.0 ** -120)
    tiny[0, 1, :, 2] = 0.0
    CC.check(fcd.crf_align_batch_raw(tiny, init[:1], y, [3]), fcd.crf_score_batch_raw(tiny, init[:1], y, [3]), tiny, init[:1],
             None, y[:, None], None, np.array([[3]]), None, 0)
    # a band whose window never reaches the last state: no alignment inside it
    xl = CC.posteriors(rng, 1, 40, 4, 5)
    yl = np.tile(np.array([1, 2, 3], np.uint8), 5)[None, :]
    pl = np.zeros((1, 15), np.uint32)  # k(t) = 15 from row 0 on: band 1 holds states 14 .. 15, out of reach by then
    got = fcd.crf_align_batch_raw(xl, init[:1], yl, [15], paths=pl, band=1)
    assert got.logp[0, 0] == -math.inf and (got.count == 0).all()
    assert fcd.crf_score_batch_raw(xl, init[:1], yl, [15], paths=pl, band=1)[0, 0] == -math.inf


def test_host_abi_optional_pointers(fcd):
    host_abi_optional_pointers(fcd, S=4)


def test_single_read_functions(fcd):
    rng = np.random.default_rng(5)
    x = CC.posteriors(rng, 1, 30, 4, 5)[0]
    init = rng.random(4).astype(np.float32)
    seq, path = fcd.crf_beam_search(x, init, "NACGT", 5)
    y = ["NACGT".index(c) for c in seq]
    rows, quals, logp = fcd.crf_align(x, init, seq, "NACGT")
    ref = R.crf_align(x, init, y)
    assert rows == ref["start"] and isinstance(logp, float) and logp_same(logp, ref["logp"])
    assert [np.float32(q) for q in quals] == ref["qual"] and all(isinstance(q, float) for q in quals)
    score = fcd.crf_score(x, init, seq, "NACGT")
    assert isinstance(score, float) and abs(score - R.crf_score(x, init, y)) <= CC.tolerance(30) and logp <= score
    assert fcd.crf_align(x, init, "", "NACGT")[:2] == ([], [])
    assert fcd.crf_align(x[:2], init, "ACGT", "NACGT") == ([], [], -math.inf)
    # multi-character labels: crf_beam_search reverses the characters of the joined string
    alpha = ["N", "Ab", "Cd", "G", "T"]
    seq2, _ = fcd.crf_beam_search(x, init, alpha, 5)
    assert seq2 != seq and fcd.crf_score(x, init, seq2, alpha) == score
    with pytest.raises(ValueError, match="alphabet size"):
        fcd.crf_score(x, init, seq, "NACG")
    with pytest.raises(ValueError, match="not a label"):
        fcd.crf_align(x, init, "AN", "NACGT")
    with pytest.raises(TypeError):
        fcd.crf_score(x, init, [1, 2], "NACGT")
    big = CC.posteriors(rng, 1, 600, 4, 5)[0]
    assert math.isfinite(fcd.crf_score(big, init, "ACGT" * 127 + "ACG", "NACGT"))  # 511 labels
    with pytest.raises(RuntimeError, match="use a band"):
        fcd.crf_score(big, init, "ACGT" * 128, "NACGT")
    with pytest.raises(RuntimeError, match="use a band"):
        fcd.crf_align(big, init, "ACGT" * 128, "NACGT")


def test_argument_errors(fcd):
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(6)
    x = CC.posteriors(rng, 2, 10, 4, 5)
    init = np.ones((2, 4), np.float32)
    labels = np.ones((2, 10), np.uint8)
    lens = np.array([3, 4], np.uint32)
    for f in (fcd.crf_align_batch_raw, fcd.crf_score_batch_raw):
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
    st, ct = np.full((2, 10), 77, np.uint32), np.full((2, 10), 77, np.uint32)
    ql, lp = np.full((2, 10), 77.0, np.float32), np.full(2, 77.0)

    def call(fn, S=4, n_hyp=1, band=0, with_path=True, start=True, count=True, with_init=True, n_init=4, out=True):
        b = nat.Batch(x.ctypes.data, 2, 10, S, 5, 200, 20, 5, 1, None)
        y = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, path.ctypes.data if with_path else None, n_hyp, 10)
        if "align" in fn:
            o = nat.Alignment(st.ctypes.data if start else None, ct.ctypes.data if count else None, ql.ctypes.data, lp.ctypes.data)
            o = C.byref(o) if out else None
        else:
            o = lp.ctypes.data if out else None
        return getattr(h.lib, fn)(h.ptr, C.byref(b), init.ctypes.data if with_init else None, n_init, 4, C.byref(y), band, o)
    for fn in ("fcd_crf_align_host", "fcd_crf_align_dev", "fcd_crf_score_host", "fcd_crf_score_dev"):
        assert call(fn, band=-1) == nat.E_INVALID
        assert call(fn, band=3, with_path=False) == nat.E_INVALID
        assert call(fn, n_hyp=0) == nat.E_INVALID
        assert call(fn, S=0) == nat.E_INVALID
        assert call(fn, with_init=False) == nat.E_INVALID
        assert call(fn, n_init=0) == nat.E_INVALID
        assert call(fn, out=False) == nat.E_INVALID
        if "align" in fn:
            assert call(fn, start=False) == nat.E_INVALID
            assert call(fn, count=False) == nat.E_INVALID
    assert (st == 77).all() and (ct == 77).all() and (ql == 77).all() and (lp == 77).all()
    assert call("fcd_crf_align_host") == nat.OK and np.isfinite(lp).all() and (ct[0, :3] == 1).all()
    lp[:] = 77.0
    assert call("fcd_crf_score_host") == nat.OK and np.isfinite(lp).all()
    # a window of 513 states: unsupported, and the message names the way out; band 64 is accepted on the same shape
    T = 512
    for fn in ("fcd_crf_align_host", "fcd_crf_score_host"):
        b = nat.Batch(None, 0, T, 4, 5, T * 20, 20, 5, 1, None)
        y = nat.Labellings(None, None, None, None, 1, T)
        out = nat.Alignment(None, None, None, None)
        o = C.byref(out) if "align" in fn else lp.ctypes.data
        assert getattr(h.lib, fn)(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(y), 0, o) == nat.E_UNSUPPORTED
        assert b"use a band" in h.lib.fcd_last_error(h.ptr)
        y = nat.Labellings(None, None, None, path.ctypes.data, 1, T)
        assert getattr(h.lib, fn)(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(y), 64, o) == nat.OK
        assert getattr(h.lib, fn)(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(y), 256, o) == nat.E_UNSUPPORTED
        b = nat.Batch(None, 0, T - 1, 4, 5, T * 20, 20, 5, 1, None)  # 512 states
        assert getattr(h.lib, fn)(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(y), 0, o) == nat.OK


def test_workspace_cap_groups(fcd):
    """a cap of one byte: every read is a launch of its own, and the arrays are the same"""
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(8)
    x = CC.posteriors(rng, 6, 40, 4, 5)
    init = rng.random((6, 4)).astype(np.float32)
    lengths = np.array([40, 17, 40, 1, 33, 40], np.int64)
    h = nat.default_handle()
    r = fcd.crf_beam_search_batch_raw(x, init, 5, 0.0, lengths=lengths)
    nb = fcd.crf_beam_search_nbest_batch_raw(x[:3], init[:3], 2, beam_size=5, lengths=lengths[:3])
    for res, xs, ins, ls in ((r, x, init, lengths), (nb, x[:3], init[:3], lengths[:3])):
        for band in (0, 4):
            whole = res.crf_align(xs, ins, lengths=ls, band=band)
            h.set_align_workspace_cap(1)
            try:
                parts = res.crf_align(xs, ins, lengths=ls, band=band)
            finally:
                h.set_align_workspace_cap(0)
            for name in ("start", "count", "qual", "logp"):
                assert np.array_equal(getattr(whole, name), getattr(parts, name), equal_nan=True), (name, band)
            assert np.isfinite(whole.logp[:, 0]).all()


def test_results_score_and_align_themselves(fcd):
    rng = np.random.default_rng(7)
    x = CC.posteriors(rng, 5, 50, 4, 5)
    init = rng.random((5, 4)).astype(np.float32)
    lengths = np.array([50, 31, 50, 1, 44], np.int64)
    r = fcd.crf_beam_search_batch_raw(x, init, 5, 0.0, lengths=lengths)
    assert (r.status == 0).all()
    for band in (0, 4):
        got, sc = r.crf_align(x, init, lengths=lengths, band=band), r.crf_score(x, init, lengths=lengths, band=band)
        assert got.logp.shape == (5, 1) and got.start.shape == (5, 1, 50) and sc.shape == (5, 1)
        CC.check(got, sc, x, init, lengths, r.labels[:, None, :], r.path[:, None, :], r.out_len[:, None], None, band)
    nb = fcd.crf_beam_search_nbest_batch_raw(x, init, 4, beam_size=6, beam_cut_threshold=0.05, lengths=lengths)
    for band in (0, 64):
        got, sc = nb.crf_align(x, init, lengths=lengths, band=band), nb.crf_score(x, init, lengths=lengths, band=band)
        assert got.logp.shape == (5, 4) and sc.shape == (5, 4)
        CC.check(got, sc, x, init, lengths, nb.labels, nb.path, nb.out_len, nb.n_hyp, band)
    # the exact score ranks the hypotheses of a read as the search's own relative scores do, where those are apart
    sc = nb.crf_score(x, init, lengths=lengths)
    for b in range(5):
        for i in range(1, int(nb.n_hyp[b])):
            if nb.score[b, i] < 0.9 * nb.score[b, i - 1]:
                assert sc[b, i] < sc[b, i - 1], (b, i)
    qs = nb.crf_align(x, init, lengths=lengths).qstrings(nb.out_len)
    assert len(qs) == 5 and all(len(q) == 4 for q in qs)
    for b in range(5):
        for i in range(4):
            assert len(qs[b][i]) == (int(nb.out_len[b, i]) if i < int(nb.n_hyp[b]) else 0)
    # a session's results are CRF results
    with fcd.CrfBeamSearchSession(5, 4, 5, init, 50) as ses:
        ses.push(x[:, :20])
        rs = ses.push(x[:, 20:], result=True)
        assert np.array_equal(rs.crf_score(x, init), fcd.crf_beam_search_batch_raw(x, init, 5, 0.0).crf_score(x, init))
    # plain CTC results are refused
    xp = CC.posteriors(rng, 2, 6, 1, 5)[:, :, 0]
    for name in ("crf_score", "crf_align"):
        with pytest.raises(ValueError, match="CRF"):
            getattr(fcd.beam_search_batch_raw(xp, 5, 0.0), name)(xp, init[:2])
        with pytest.raises(ValueError, match="CRF"):
            getattr(fcd.beam_search_nbest_batch_raw(xp, 2, 5, 0.0), name)(xp, init[:2])


def test_crf_beam_search_qstring(fcd):
    rng = np.random.default_rng(9)
    x = CC.posteriors(rng, 1, 60, 4, 5)[0]
    init = rng.random(4).astype(np.float32)
    plain = fcd.crf_beam_search(x, init, "NACGT", 5, 0.0)
    seq, path = fcd.crf_beam_search(x, init, "NACGT", 5, 0.0, qstring=True)
    n = len(plain[0])
    assert n > 0 and path == plain[1] and seq[:n] == plain[0] and len(seq) == 2 * n
    _, quals, _ = fcd.crf_align(x, init, plain[0], "NACGT")
    lib = fcd._native.load()
    assert seq[n:] == "".join(chr(lib.fcd_phred(q, 1.0, 0.0)) for q in quals)
    biased = fcd.crf_beam_search(x, init, "NACGT", 5, 0.0, qstring=True, qscale=2.0, qbias=1.5)[0]
    assert biased[:n] == plain[0] and biased[n:] == "".join(chr(lib.fcd_phred(q, 2.0, 1.5)) for q in quals)
    with pytest.raises(TypeError):
        fcd.crf_beam_search(x, init, "NACGT", 5, 0.0, True)  # the new arguments are keyword-only
    # a result of more than 511 labels: aligned at band 64 around the search's own path
    long_x = CC.greedy_posteriors(rng, 1, 200, 4, 5)[0]
    long_x = np.concatenate([long_x] * 9)  # 1800 rows, about 630 labels
    lseq, lpath = fcd.crf_beam_search(long_x, init, "NACGT", 5, 0.0, qstring=True)
    ln = len(lpath)
    assert ln > 511 and len(lseq) == 2 * ln
    fcd.set_coalescing(8)
    try:
        assert fcd.crf_beam_search(x, init, "NACGT", 5, 0.0, qstring=True) == (seq, path)
        assert fcd.crf_beam_search(x, init, "NACGT", 5, 0.0) == plain
    finally:
        fcd.set_coalescing(0)
