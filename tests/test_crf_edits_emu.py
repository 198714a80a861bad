"""CPU-side check of the CRF deletion and insertion walks (csrc/crf_posterior.hip, compiled against tests/hipemu's lockstep
wave64 emulation) through crf_edits_batch_raw on numpy, against the restatements of tests/crf_edits_reference.py: the shapes
of tests/crf_posterior_cases.py (every K at the exact windows of 64 .. 512 states, histories of 1 / 2 / 3 / 5 labels, N = 3 /
5 / 9, both staging regimes, f16 / bf16, time-major strides, ragged lengths, n_hyp = 3 with n_valid, bands 1 / 4 / 64, the
slot-ring wrap), the one-row table S = 1, short labellings whose chains are cut by the end, every edge row of include/fcd.h
with a NaN only variants read, edits heavier than the labelling by more than 2^130, EditResult.best's pick against crf_score,
the argument errors and limits, the results' own crf_edits, the single-read function, and a workspace limit that forces
several groups.  The -m gpu twin is tests/test_gpu_crf_edits.py."""
import math

import numpy as np
import pytest

import crf_edits_cases as EC
import crf_edits_reference as ER
import crf_lattice_cases as CC
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("case", EC.CASES, ids=[c[0] for c in EC.CASES])
def test_against_restatements(fcd, case):
    EC.run_case(fcd, EC.build_case(case))


@pytest.mark.parametrize("S,N", [(1, 5), (4, 5), (16, 5), (64, 5), (1024, 5), (8, 3), (8, 9)])
def test_short_labellings(fcd, S, N):
    """L = 0 .. 6 at T = 9 (S = 1: labellings of 1s, the last label free): chains cut by the end, T_r close to L"""
    rng = np.random.default_rng(50 + S + N)
    T, B = 9, 7
    x = CC.posteriors(rng, B, T, S, N)
    init = rng.random((B, S)).astype(np.float32)
    labels = np.zeros((B, T), np.uint8)
    lens = np.arange(B).astype(np.uint32)
    lengths = np.array([9, 9, 3, 4, 4, 9, 6], np.int64)
    for b in range(B):
        labels[b, :lens[b]] = 1 if S == 1 else rng.integers(1, N, lens[b])
    if S == 1:
        labels[3, 2], labels[5, 4] = 3, 2
    got = EC.edits(fcd, None, x, init, labels, lens, lengths)
    for b in range(B):
        n, Tr = int(lens[b]), int(lengths[b])
        ref = EC.reference_one(x[b, :Tr], init[b], labels[b, :n], 0, None)
        assert math.isfinite(ref["chain"][2])
        EC.check_one(got.deletion[b, 0, :n], got.insertion[b, 0, :n + 1], ref, Tr, ("short", S, N, "L", n))


def test_edge_rows(fcd):
    EC.edge_rows(fcd)


def test_heavy_variants(fcd):
    EC.heavy_variants(fcd)


def test_best_edit_is_crf_score(fcd):
    EC.best_edit_is_crf_score(fcd)


def test_argument_errors_and_limits(fcd):
    EC.argument_errors(fcd)
    x = CC.posteriors(np.random.default_rng(1), 1, 12, 5, 4)
    from fast_ctc_decode_amd import _native as nat
    with pytest.raises(nat.NativeError) as e:
        fcd.crf_edits_batch_raw(x, np.ones((1, 5), np.float32), np.ones((1, 12), np.uint8), [5])
    assert e.value.code == nat.E_UNSUPPORTED and "crf_edits" in str(e.value) and "power of N - 1" in str(e.value)
    with pytest.raises(ValueError):
        fcd.crf_edits_batch_raw(x, np.ones((1, 5), np.float32), np.ones((1, 12), np.uint8), [5], band=3)  # no paths


def test_results_give_their_edits(fcd):
    rng = np.random.default_rng(7)
    x = CC.posteriors(rng, 4, 40, 4, 5)
    init = rng.random((4, 4)).astype(np.float32)
    lengths = np.array([40, 23, 1, 36], np.int64)
    r = fcd.crf_beam_search_batch_raw(x, init, 5, 0.0, lengths=lengths)
    for band in (0, 4):
        got = r.crf_edits(x, init, lengths=lengths, band=band)
        assert got.deletion.shape == (4, 1, 40) and got.insertion.shape == (4, 1, 41, 4) and got.logp.shape == (4, 1)
        for b in range(4):
            n = int(r.out_len[b])
            ref = EC.reference_one(x[b, :lengths[b]], init[b], r.labels[b, :n], band, r.path[b, :n] if band else None)
            EC.check_one(got.deletion[b, 0, :n], got.insertion[b, 0, :n + 1], ref, int(lengths[b]), ("BatchResult", band, b))
    nb = fcd.crf_beam_search_nbest_batch_raw(x, init, 3, beam_size=5, lengths=lengths)
    g = nb.crf_edits(x, init, lengths=lengths, band=64)
    assert g.deletion.shape == (4, 3, 40) and g.insertion.shape == (4, 3, 41, 4)
    for b in range(4):
        for i in range(3):
            n = int(nb.out_len[b, i])
            if i >= int(nb.n_hyp[b]):
                assert math.isnan(g.logp[b, i]) and np.isnan(g.deletion[b, i, :n]).all()
                continue
            ref = EC.reference_one(x[b, :lengths[b]], init[b], nb.labels[b, i, :n], 64, nb.path[b, i, :n])
            assert abs(g.logp[b, i] - ref["chain"][2]) <= CC.tolerance(int(lengths[b]))
            EC.check_one(g.deletion[b, i, :n], g.insertion[b, i, :n + 1], ref, int(lengths[b]), ("NBestResult", b, i))
    # plain CTC results are refused, and ctc_edits keeps refusing CRF results
    xp = CC.posteriors(rng, 2, 6, 1, 5)[:, :, 0]
    with pytest.raises(ValueError, match="CRF"):
        fcd.beam_search_batch_raw(xp, 5, 0.0).crf_edits(xp, init[:2])
    with pytest.raises(ValueError, match="CRF"):
        fcd.beam_search_nbest_batch_raw(xp, 2, 5, 0.0).crf_edits(xp, init[:2])
    with pytest.raises(ValueError, match="CRF"):
        r.ctc_edits(x)
    with pytest.raises(ValueError, match="CRF"):
        nb.ctc_edits(x)


def test_single_read_function(fcd):
    rng = np.random.default_rng(5)
    x = CC.posteriors(rng, 1, 30, 4, 5)[0]
    init = rng.random(4).astype(np.float32)
    seq, _ = fcd.crf_beam_search(x, init, "NACGT", 5)
    dele, ins, logp = fcd.crf_edits(x, init, seq, "NACGT")
    y = ["NACGT".index(c) for c in seq]
    ref = EC.reference_one(x, init, y, 0, None)
    assert dele.shape == (len(seq),) and ins.shape == (len(seq) + 1, 4) and dele.dtype == np.float32 and isinstance(logp, float)
    assert abs(logp - fcd.crf_score(x, init, seq, "NACGT")) <= 2.0 ** -40 * abs(logp)
    EC.check_one(dele, ins, ref, 30, "single read")
    d0, i0, lp0 = fcd.crf_edits(x, init, "", "NACGT")
    assert d0.shape == (0,) and i0.shape == (1, 4) and math.isfinite(lp0) and np.isfinite(i0).all()
    EC.compare(i0, ER.rescored(x, init, [])[1], lp0, 30, "the empty labelling")
    dn, inn, lpi = fcd.crf_edits(x[:2], init, "ACGT", "NACGT")
    assert lpi == -math.inf and np.isnan(dn).all() and np.isnan(inn).all()
    with pytest.raises(ValueError, match="alphabet size"):
        fcd.crf_edits(x, init, seq, "NACG")
    with pytest.raises(ValueError, match="not a label"):
        fcd.crf_edits(x, init, "AN", "NACGT")


def test_workspace_limit_groups(fcd):
    EC.workspace_limit_groups(fcd)
