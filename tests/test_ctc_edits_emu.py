"""CPU-side check of the edit-likelihood kernels (csrc/ctc_posterior.hip: edit_back_kernel, compiled against
tests/hipemu's lockstep wave64 emulation) through ctc_edits_batch_raw on numpy, against the restatement
tests/ctc_edits_reference.py: the cases of tests/ctc_edits_cases.py, every edge row of include/fcd.h, consistency with
ctc_score of the edited labellings, EditResult.best, the argument errors and the limits at both layers, the results' own
ctc_edits and the single-read function.  The -m gpu twin is tests/test_gpu_ctc_edits.py."""
import ctypes as C
import math

import numpy as np
import pytest

import ctc_edits_cases as EC
import ctc_edits_reference as ER
import ctc_posterior_cases as PC
import ctc_score_cases as SC
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("case", EC.CASES, ids=[c[0] for c in EC.CASES])
def test_against_restatement(fcd, case):
    EC.run_case(fcd, EC.build_case(fcd, case))


def test_edge_rows(fcd):
    """through fcd_ctc_edits_dev into sentinel-filled outputs: every entry k < len, g <= len is written, no other"""
    from fast_ctc_decode_amd import _native as nat
    x, labels, lens, lengths = PC.edge_batch()
    dele, ins, lp = np.full((10, 8), 77.0, np.float32), np.full((10, 9, 3), 77.0, np.float32), np.full(10, 77.0)
    h = nat.default_handle()
    b = nat.Batch(x.ctypes.data, 10, 6, 1, 4, 24, 4, 0, 1, lengths.ctypes.data)
    y = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, None, 1, 8)
    out = nat.Edits(dele.ctypes.data, ins.ctypes.data, lp.ctypes.data)
    assert h.lib.fcd_ctc_edits_dev(h.ptr, C.byref(b), C.byref(y), 1, 0, C.byref(out)) == nat.OK
    EC.check_edges(dele, ins, lp, x, labels, lens, lengths, 77.0)
    # _host: the entries beyond the labelling come back as 0
    got = fcd.ctc_edits_batch_raw(x, labels, lens, lengths=lengths)
    EC.check_edges(got.deletion[:, 0], got.insertion[:, 0], got.logp[:, 0], x, labels, lens, lengths, 0.0)
    # i >= n_valid: NaN logp, and NaN for the entries the row claims to hold
    lab2, len2 = np.stack([labels, labels], 1), np.stack([lens, lens], 1)
    got2 = fcd.ctc_edits_batch_raw(x, lab2, len2, lengths=lengths, n_valid=np.ones(10, np.uint32))
    assert np.array_equal(got2.deletion[:, 0], got.deletion[:, 0], equal_nan=True) and np.isnan(got2.logp[:, 1]).all()
    assert np.array_equal(got2.insertion[:, 0], got.insertion[:, 0], equal_nan=True)
    assert np.isnan(got2.deletion[8, 1, :3]).all() and (got2.deletion[8, 1, 3:] == 0).all()
    assert np.isnan(got2.insertion[8, 1, :4]).all() and (got2.insertion[8, 1, 4:] == 0).all()
    # every row emits (collapse_repeats = 0): read 7 has an alignment, one row per label
    nc = fcd.ctc_edits_batch_raw(x, labels, lens, False, lengths)
    d, i, rlp = ER.ctc_edits(x[7], labels[7, :4], False)
    assert SC.same(nc.logp[7, 0], rlp, 6)
    EC.check_one(nc.deletion[7, 0, :4], d, 6, "no collapse, read 7, deletion")
    EC.check_one(nc.insertion[7, 0, :5], i, 6, "no collapse, read 7, insertion")
    # a NaN posterior in a column the labelling does not read, at a row every gap is live at: logp and the deletions
    # stand, the insertions of that label are NaN
    rng = np.random.default_rng(9)
    xn = SC.posteriors(rng, 1, 12, 4)
    xn[0, 5, 2] = np.nan
    yn = np.array([[1, 1, 3]], np.uint8)
    gn = fcd.ctc_edits_batch_raw(xn, yn, [3])
    d, i, rlp = ER.ctc_edits(xn[0], yn[0])
    assert math.isfinite(rlp) and SC.same(gn.logp[0, 0], rlp, 12) and np.isnan(i[:, 1]).all() and np.isfinite(d).all()
    EC.check_one(gn.deletion[0, 0, :3], d, 12, "NaN in a variant's column, deletion")
    EC.check_one(gn.insertion[0, 0, :4], i, 12, "NaN in a variant's column, insertion")
    # very small posteriors (the row maximum falls by 2^-100 in one step): nothing is lost
    tiny = x[8:9].copy()
    tiny[0, 2, :] *= np.float32(2.0 ** -100)
    tiny[0, 4, :] *= np.float32(2.0 ** -120)
    gt = fcd.ctc_edits_batch_raw(tiny, labels[8:9], lens[8:9])
    d, i, _ = ER.ctc_edits(tiny[0], labels[8, :3])
    EC.check_one(gt.deletion[0, 0, :3], d, 6, "tiny rows, deletion")
    EC.check_one(gt.insertion[0, 0, :4], i, 6, "tiny rows, insertion")


def test_stray_nan_and_inf(fcd):
    """a NaN or an infinity in a cell that only a shortened labelling reads stays out of logp and of every other entry"""
    for x, y, bad in EC.stray_cases():
        got = fcd.ctc_edits_batch_raw(x[None], y[None], [3])
        score = fcd.ctc_score_batch_raw(x[None], y[None], [3])[0, 0]
        post = fcd.ctc_posterior_batch_raw(x[None], y[None], [3])
        assert post.logp[0, 0] == score  # (the substitution posteriors' forward pass is ctc_score's, bit for bit)
        EC.check_stray(got.deletion[0, 0, :3], got.insertion[0, 0, :4], got.logp[0, 0], score, x, y, bad)


def test_consistent_with_ctc_score(fcd):
    """exact mode: exp(deletion[k]) P(y) is ctc_score of the shortened labelling, one insertion per labelling ctc_score of
    the lengthened one -- each within the sum of the two tolerances"""
    rng = np.random.default_rng(10)
    x = SC.posteriors(rng, 4, 30, 5)
    lengths = np.array([30, 17, 8, 26], np.int64)
    r = fcd.beam_search_batch_raw(x, 5, 0.0, lengths=lengths)
    got = r.ctc_edits(x, lengths=lengths)
    assert got.deletion.shape == (4, 1, 30) and got.insertion.shape == (4, 1, 31, 4) and got.logp.shape == (4, 1)
    for b in range(4):
        n, Tr = int(r.out_len[b]), int(lengths[b])
        y = r.labels[b, :n].tolist()
        variants = [(y[:k] + y[k + 1:], float(got.deletion[b, 0, k])) for k in range(n)]
        g, c = int(rng.integers(n + 1)), int(rng.integers(1, 5))
        variants.append((y[:g] + [c] + y[g:], float(got.insertion[b, 0, g, c - 1])))
        lab = np.zeros((len(variants), 31), np.uint8)
        for j, (v, _) in enumerate(variants):
            lab[j, :len(v)] = v
        sc = fcd.ctc_score_batch_raw(np.repeat(x[b:b + 1], len(variants), 0), lab, [len(v) for v, _ in variants],
                                     lengths=np.full(len(variants), Tr))
        for j, (v, ratio) in enumerate(variants):
            want = sc[j, 0] - got.logp[b, 0]
            if math.isinf(want):
                assert ratio == want
            elif want >= EC.FLOOR:
                assert abs(ratio - want) <= EC.tolerance(Tr, want) + 2 * SC.tolerance(Tr), (b, j, ratio, want)


def test_best_edit(fcd):
    """EditResult.best against an argmax over the restatement, substitutions included"""
    import ctc_posterior_reference as PR
    rng = np.random.default_rng(11)
    x = SC.posteriors(rng, 6, 24, 5)
    r = fcd.beam_search_batch_raw(x, 5, 0.0)
    labels, lens = r.labels.copy(), r.out_len.copy()
    for b in range(1, 6):  # spoil five of the six labellings by one edit each, so that an edit is worth making
        n = int(lens[b])
        lab, _ = SC.edit(rng, labels[b, :n].tolist(), list(range(n)), 5, 24)
        labels[b] = 0
        labels[b, :len(lab)] = lab
        lens[b] = len(lab)
    ed = fcd.ctc_edits_batch_raw(x, labels, lens)
    po = fcd.ctc_posterior_batch_raw(x, labels, lens)
    plain = ed.best(lens)
    full = ed.best(lens, po, labels)
    assert all(a.shape == (6, 1) for a in plain + full)
    compared = 0
    for b in range(6):
        n = int(lens[b])
        d, ins, lp = ER.ctc_edits(x[b], labels[b, :n])
        post, _ = PR.ctc_posterior(x[b], labels[b, :n])
        with np.errstate(all="ignore"):
            sub = np.log(post) - np.log(post[np.arange(n), labels[b, :n].astype(int) - 1])[:, None]
        sub[np.arange(n), labels[b, :n].astype(int) - 1] = -np.inf
        y = labels[b, :n]
        # (a substitution's log-ratio is the logarithm of a ratio of two posteriors, each within 16 T 2^-24 of its value)
        for got, sb, extra in ((plain, None, 0.0), (full, sub, 32 * 24 * 2.0 ** -24)):
            want, want_val, decided = EC.best_variant(y, d, ins, 24, sb, extra)
            if not decided:
                continue
            compared += 1
            have = EC.apply_edit(y, int(got[0][b, 0]), int(got[1][b, 0]), int(got[2][b, 0]))
            assert have == want, (b, want, [a[b, 0] for a in got])
            assert abs(got[3][b, 0] - want_val) <= EC.tolerance(24, want_val) + extra
    print("ctc_edits: best edit compared on %d of 12 (labelling, with / without substitutions) pairs" % compared)
    assert compared >= 10
    assert (np.asarray(full[3]) >= np.asarray(plain[3])).all() and (np.asarray(plain[0])[1:] != 0).any()
    with pytest.raises(ValueError, match="labels"):
        ed.best(lens, po)


def test_argument_errors_and_limits(fcd):
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(6)
    x = SC.posteriors(rng, 2, 10, 5)
    labels = np.ones((2, 10), np.uint8)
    lens = np.array([3, 4], np.uint32)
    with pytest.raises(ValueError):
        fcd.ctc_edits_batch_raw(x, labels, lens, band=-1)
    with pytest.raises(ValueError):
        fcd.ctc_edits_batch_raw(x, labels, lens, band=4)  # no paths
    with pytest.raises(TypeError):
        fcd.ctc_edits_batch_raw(x, labels, lens, band=1.5)
    with pytest.raises(ValueError):
        fcd.ctc_edits_batch_raw(x, labels[:1], lens)
    with pytest.raises(ValueError):
        fcd.ctc_edits_batch_raw(x, labels, lens, paths=np.zeros((2, 9), np.uint32), band=2)
    # the C ABI refuses them itself, before anything is enqueued or written
    h = nat.default_handle()
    path = np.zeros((2, 10), np.uint32)
    de, ins, lp = np.full((2, 10), 77.0, np.float32), np.full((2, 11, 4), 77.0, np.float32), np.full(2, 77.0)

    def call(S=1, n_hyp=1, band=0, with_path=True, fn="fcd_ctc_edits_host", deletion=True, insertion=True, logp=True):
        b = nat.Batch(x.ctypes.data, 2, 10, S, 5, 50, 5, 0, 1, None)
        y = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, path.ctypes.data if with_path else None, n_hyp, 10)
        out = nat.Edits(de.ctypes.data if deletion else None, ins.ctypes.data if insertion else None,
                        lp.ctypes.data if logp else None)
        return getattr(h.lib, fn)(h.ptr, C.byref(b), C.byref(y), 1, band, C.byref(out))
    for fn in ("fcd_ctc_edits_host", "fcd_ctc_edits_dev"):
        assert call(band=-1, fn=fn) == nat.E_INVALID
        assert call(band=3, with_path=False, fn=fn) == nat.E_INVALID
        assert call(n_hyp=0, fn=fn) == nat.E_INVALID
        assert call(S=4, fn=fn) == nat.E_INVALID
        assert call(deletion=False, fn=fn) == nat.E_INVALID
        assert call(insertion=False, fn=fn) == nat.E_INVALID
        b = nat.Batch(x.ctypes.data, 2, 10, 1, 5, 50, 5, 0, 1, None)
        y = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, None, 1, 10)
        assert getattr(h.lib, fn)(h.ptr, C.byref(b), C.byref(y), 1, 0, None) == nat.E_INVALID
    assert (de == 77).all() and (ins == 77).all() and (lp == 77).all()
    assert call(logp=False) == nat.OK and (lp == 77).all() and np.isfinite(de[0, :3]).all()  # (logp is optional)
    assert call() == nat.OK and np.isfinite(lp).all()
    # the limits: unsupported, and the message names ctc_edits and the way out
    for T, N, band, msg in ((255, 5, 0, b"use a band"), (600, 5, 127, b"narrower band"), (40, 11, 0, b"8 labels"),
                            (40000, 5, 4, b"smaller stride")):
        b = nat.Batch(None, 0, T, 1, N, T * N, N, 0, 1, None)
        y = nat.Labellings(None, None, None, path.ctypes.data, 1, T)
        assert h.lib.fcd_ctc_edits_host(h.ptr, C.byref(b), C.byref(y), 1, band, C.byref(nat.Edits(None, None, None))) == nat.E_UNSUPPORTED
        assert msg in h.lib.fcd_last_error(h.ptr) and b"ctc_edits" in h.lib.fcd_last_error(h.ptr), h.lib.fcd_last_error(h.ptr)
    for T, band in ((254, 0), (600, 126)):  # 509 and 507 states: the widest windows there are below 511
        b = nat.Batch(None, 0, T, 1, 5, T * 5, 5, 0, 1, None)
        y = nat.Labellings(None, None, None, path.ctypes.data, 1, T)
        assert h.lib.fcd_ctc_edits_host(h.ptr, C.byref(b), C.byref(y), 1, band, C.byref(nat.Edits(None, None, None))) == nat.OK
    with pytest.raises(nat.NativeError) as e:  # 511 states
        fcd.ctc_edits_batch_raw(SC.posteriors(rng, 1, 255, 5), np.ones((1, 255), np.uint8), [5])
    assert e.value.code == nat.E_UNSUPPORTED and "use a band" in str(e.value)
    with pytest.raises(nat.NativeError) as e:  # N - 1 = 9
        fcd.ctc_edits_batch_raw(SC.posteriors(rng, 1, 20, 10), np.ones((1, 20), np.uint8), [5])
    assert e.value.code == nat.E_UNSUPPORTED


def test_results_score_themselves(fcd):
    rng = np.random.default_rng(7)
    x = SC.posteriors(rng, 4, 30, 5)
    lengths = np.array([30, 17, 1, 26], np.int64)
    r = fcd.beam_search_batch_raw(x, 5, 0.0, lengths=lengths)
    for band in (0, 4):
        got = r.ctc_edits(x, lengths=lengths, band=band)
        for b in range(4):
            n, Tr = int(r.out_len[b]), int(lengths[b])
            d, i, lp = ER.ctc_edits(x[b, :Tr], r.labels[b, :n], True, band, r.path[b, :n] if band else None)
            assert SC.same(got.logp[b, 0], lp, Tr)
            EC.check_one(got.deletion[b, 0, :n], d, Tr, ("BatchResult", band, b, "deletion"))
            EC.check_one(got.insertion[b, 0, :n + 1], i, Tr, ("BatchResult", band, b, "insertion"))
    nb = fcd.beam_search_nbest_batch_raw(x, 3, beam_size=5, lengths=lengths)
    g = nb.ctc_edits(x, lengths=lengths, band=64)
    assert g.deletion.shape == (4, 3, 30) and g.insertion.shape == (4, 3, 31, 4)
    for b in range(4):
        for i in range(3):
            if i >= int(nb.n_hyp[b]):
                assert math.isnan(g.logp[b, i])
                continue
            n, Tr = int(nb.out_len[b, i]), int(lengths[b])
            d, ins, lp = ER.ctc_edits(x[b, :Tr], nb.labels[b, i, :n], True, 64, nb.path[b, i, :n])
            EC.check_one(g.deletion[b, i, :n], d, Tr, ("NBestResult", b, i, "deletion"))
            EC.check_one(g.insertion[b, i, :n + 1], ins, Tr, ("NBestResult", b, i, "insertion"))
    xc = np.abs(rng.standard_normal((2, 6, 4, 5))).astype(np.float32)
    init = np.ones((2, 4), np.float32)
    with pytest.raises(ValueError, match="CRF"):
        fcd.crf_beam_search_batch_raw(xc, init, 5, 0.0).ctc_edits(xc)
    with pytest.raises(ValueError, match="CRF"):
        fcd.crf_beam_search_nbest_batch_raw(xc, init, 2, 5, 0.0).ctc_edits(xc)


def test_single_read_function(fcd):
    rng = np.random.default_rng(5)
    x = SC.posteriors(rng, 1, 30, 5)[0]
    seq, _ = fcd.beam_search(x, "NACGT", 5)
    dele, ins, logp = fcd.ctc_edits(x, seq, "NACGT")
    d, i, lp = ER.ctc_edits(x, ["NACGT".index(c) for c in seq])
    assert dele.shape == (len(seq),) and ins.shape == (len(seq) + 1, 4) and dele.dtype == ins.dtype == np.float32
    assert isinstance(logp, float) and SC.same(logp, lp, 30)
    EC.check_one(dele, d, 30, "single read, deletion")
    EC.check_one(ins, i, 30, "single read, insertion")
    d0, i0, lp0 = fcd.ctc_edits(x, "", "NACGT")
    assert d0.shape == (0,) and i0.shape == (1, 4) and math.isfinite(lp0)
    EC.check_one(i0, ER.ctc_edits(x, [])[1], 30, "the empty string")
    dn, inn, lpi = fcd.ctc_edits(x[:2], "ACGT", "NACGT")
    assert lpi == -math.inf and np.isnan(dn).all() and np.isnan(inn).all()
    with pytest.raises(ValueError, match="not a label"):
        fcd.ctc_edits(x, "AN", "NACGT")


def test_workspace_limit_groups(fcd):
    """a workspace limit of one byte: every read is a launch pair of its own, in the same memory; the same values"""
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(8)
    x = SC.posteriors(rng, 5, 40, 5)
    lengths = np.array([40, 17, 40, 1, 33], np.int64)
    h = nat.default_handle()
    nb = fcd.beam_search_nbest_batch_raw(x, 2, beam_size=5, lengths=lengths)
    for band in (0, 4):
        whole = nb.ctc_edits(x, lengths=lengths, band=band)
        h.set_workspace_limit(1)
        try:
            parts = nb.ctc_edits(x, lengths=lengths, band=band)
        finally:
            h.set_workspace_limit(0)
        assert np.array_equal(whole.deletion, parts.deletion, equal_nan=True)
        assert np.array_equal(whole.insertion, parts.insertion, equal_nan=True)
        assert np.array_equal(whole.logp, parts.logp, equal_nan=True) and np.isfinite(whole.logp[:, 0]).all()
