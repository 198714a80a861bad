"""CPU-side check of the CRF Viterbi walk (csrc/crf_viterbi.hip, crf_viterbi_kernel, compiled against
tests/hipemu's lockstep wave64 emulation) through crf_viterbi_search_batch_raw on numpy, against the restatement
tests/crf_viterbi_reference.py: the grid of tests/crf_viterbi_cases.py (S = 4 .. 1024 and the non-power multiple 12, N = 2 /
3 / 5 / 9, T = 1 .. 300 around the 64-emission flush of the traceback, ragged lengths with an empty read, f32 / f16 / bf16,
time-major strides), every edge case of the definition, the argument errors at both layers, every combination of the C
ABI's nullable pointers, a workspace cap that forces several launch groups, the cross-checks against crf_align / crf_score /
crf_greedy_search, and the single-read and batch string functions.  The -m gpu twin is tests/test_gpu_crf_viterbi.py."""
import numpy as np
import pytest

import crf_lattice_cases as CC
import crf_viterbi_cases as VC
import crf_viterbi_reference as R
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("case", VC.CASES, ids=[c[0] for c in VC.CASES])
def test_against_restatement(fcd, case):
    VC.run_case(fcd, VC.build_case(case))


def test_edge_cases(fcd):
    VC.edge_cases(fcd)


def test_tie_rules(fcd):
    VC.tie_rules(fcd)


def test_argument_errors_and_limits(fcd):
    VC.argument_errors(fcd)


def test_nullable_outputs(fcd):
    VC.nullable_outputs(fcd)


def test_workspace_cap_groups(fcd):
    VC.workspace_groups(fcd)


def test_peaked_rows_give_greedys_result(fcd):
    """where greedy's path is the optimum (tests/test_crf_viterbi_reference.py), the two kernels agree exactly"""
    rng = np.random.default_rng(21)
    x = CC.greedy_posteriors(rng, 4, 200, 16, 5)
    init = rng.random((4, 16)).astype(np.float32)
    lengths = np.array([200, 130, 64, 1], np.int64)
    v = fcd.crf_viterbi_search_batch_raw(x, init, lengths, qual=True)
    g = fcd.crf_greedy_search_batch_raw(x, init, lengths, qual=True)
    for b in range(4):
        n = int(g.out_len[b])
        assert int(v.out_len[b]) == n and np.array_equal(v.labels[b, :n], g.labels[b, :n])
        assert np.array_equal(v.path[b, :n], g.path[b, :n]) and np.array_equal(v.qual[b, :n].view(np.uint32), g.qual[b, :n].view(np.uint32))


def test_result_type_and_string_functions(fcd):
    from fast_ctc_decode_amd import api
    rng = np.random.default_rng(4)
    x = np.stack([R.random_case(rng, 30, 4, 5)[0] for _ in range(3)])
    init = rng.random((3, 4)).astype(np.float32)
    r = fcd.crf_viterbi_search_batch_raw(x, init)
    assert isinstance(r, api._CrfBatchResult) and r.qual is None and r.logp.shape == (3,)
    assert r.crf_posterior(x, init).post.shape == (3, 1, 30, 4) and r.crf_edits(x, init).deletion.shape == (3, 1, 30)
    with pytest.raises(ValueError, match="CRF"):
        r.ctc_score(x)
    batch = fcd.crf_viterbi_search_batch(x, init, "NACGT", qstring=True, qscale=1.5, qbias=0.5)
    for b in range(3):
        ref = R.viterbi(x[b], init[b])
        seq, path = fcd.crf_viterbi_search(x[b], init[b], "NACGT")
        assert seq == "".join("NACGT"[l] for l in ref["labels"]) and path == ref["path"]
        sq, pq = fcd.crf_viterbi_search(x[b], init[b], "NACGT", qstring=True, qscale=1.5, qbias=0.5)
        assert sq[:len(seq)] == seq and len(sq) == 2 * len(seq) and pq == path
        assert sq[len(seq):] == api._qual_chars(ref["qual"], 1.5, 0.5)
        assert batch[b] == (sq, path)
    assert fcd.crf_viterbi_search_batch(x, init, "NACGT", lengths=[30, 2, 0], paths=None)[2] == ("", None)
    with pytest.raises(ValueError, match="alphabet size"):
        fcd.crf_viterbi_search(x[0], init[0], "NACG")
    with pytest.raises(ValueError, match="Empty alphabet"):
        fcd.crf_viterbi_search(x[0], init[0], "")
    with pytest.raises(RuntimeError, match="empty"):
        fcd.crf_viterbi_search(x[0][:0], init[0], "NACGT")
    bad = init[0].copy()
    bad[1] = np.nan
    with pytest.raises(RuntimeError):
        fcd.crf_viterbi_search(x[0], bad, "NACGT")
