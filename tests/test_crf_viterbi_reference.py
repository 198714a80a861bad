"""CPU-only: the restatement of the CRF Viterbi search (tests/crf_viterbi_reference.py, the specification of
fcd_crf_viterbi_search_* in include/fcd.h) against the float64 enumeration of all N^T label sequences of tiny cases, against
crf_greedy_search's own path (a lower bound), and on peaked posteriors, where greedy's path is the optimum."""
import math

import numpy as np
import pytest

import crf_lattice_cases as CC
import crf_viterbi_reference as R

GRID = [(4, 5, 4), (16, 5, 4), (4, 3, 6), (2, 3, 6), (12, 5, 4), (8, 5, 4), (3, 2, 7), (6, 4, 5)]
SEEDS = 40


def _case(S, N, T, seed):
    return R.random_case(np.random.default_rng(1000 * S + 100 * N + seed), T, S, N)


@pytest.mark.parametrize("S,N,T", GRID)
def test_restatement_is_the_enumerations_best(S, N, T):
    """labels and path equal the best of all N^T sequences, logp within 4 T 2^-24 (T products of one rounding each, and the
    posteriors' own conversion is exact); every seed's best and second best differ by more than 1e-6 relative, so every seed
    proves something"""
    tol = 4 * T * 2.0 ** -24
    for seed in range(SEEDS):
        p, init = _case(S, N, T, seed)
        got = R.viterbi(p, init)
        every = R.enumerate_paths(p, init)
        assert len(every) == N ** T
        (w0, labels, path), w1 = every[0], every[1][0]
        assert (w0 - w1) / w0 >= 1e-6, ("a near tie proves nothing: replace the seed", S, N, T, seed)
        assert got["status"] == 0 and got["labels"] == labels and got["path"] == path, (S, N, T, seed)
        assert abs(got["logp"] - math.log(w0)) <= tol, (S, N, T, seed, got["logp"], math.log(w0))
        # qual: the posterior of each emission along the state trajectory of the labels
        s = R.first_max(init)
        for k, (t, a) in enumerate(zip(path, labels)):
            assert got["qual"][k] == p[t, s, a]
            s = (s * (N - 1)) % S + (a - 1)


@pytest.mark.parametrize("S,N,T", GRID + [(64, 5, 40), (1024, 5, 12), (16, 3, 300)])
def test_no_worse_than_greedy(S, N, T):
    tol = 4 * T * 2.0 ** -24
    for seed in range(8):
        p, init = _case(S, N, T, seed)
        got = R.viterbi(p, init)
        _, _, _, logw = R.greedy(p, init)
        assert got["logp"] >= logw - tol, (S, N, T, seed, got["logp"], logw)


@pytest.mark.parametrize("S,N,T", [(16, 5, 500), (4, 5, 63), (64, 9, 100), (12, 5, 65), (4, 2, 300)])
def test_peaked_rows_give_greedys_path(S, N, T):
    """every row's maximum >= 0.99, every other value <= 0.001, T <= 500: any deviation from greedy's path costs a factor
    <= 0.001 < 0.99^500, so greedy's path is the optimum: labels, path and qual are equal exactly"""
    assert T <= 500 and 0.001 < 0.99 ** 500
    rng = np.random.default_rng(S + N + T)
    x = CC.greedy_posteriors(rng, 3, T, S, N)
    srt = np.sort(x, -1)
    assert (srt[..., -1] >= 0.99).all() and (srt[..., -2] <= 0.001).all()
    init = rng.random((3, S)).astype(np.float32)
    for b in range(3):
        got = R.viterbi(x[b], init[b])
        labels, path, qual, logw = R.greedy(x[b], init[b])
        assert got["labels"] == labels and got["path"] == path
        assert np.asarray(got["qual"], np.float32).view(np.uint32).tolist() == np.asarray(qual, np.float32).view(np.uint32).tolist()
        assert abs(got["logp"] - logw) <= 4 * T * 2.0 ** -24


def test_edge_rows_of_the_definition():
    p, init = _case(4, 5, 6, 0)
    assert R.viterbi(p[:0], init) == dict(status=0, labels=[], path=[], qual=[], logp=0.0)
    bad = init.copy()
    bad[2] = np.nan
    assert R.viterbi(p, bad)["status"] == R.ST_BAD_STATE and R.viterbi(p[:0], bad)["status"] == R.ST_BAD_STATE
    assert R.viterbi(p, np.zeros(0, np.float32))["status"] == R.ST_BAD_STATE
    assert R.viterbi(p, np.array([0, 0, 0, 0, 1], np.float32))["status"] == R.ST_BAD_STATE
    q = p.copy()
    q[3, 1, 2] = np.nan
    got = R.viterbi(q, init)
    assert got["status"] == R.ST_INCOMPARABLE and got["labels"] == [] and math.isnan(got["logp"])
    # ties: stay before advance, the lowest i among advances, the first maximum at the end
    flat = np.full((3, 4, 5), 0.25, np.float32)
    got = R.viterbi(flat, np.array([0, 1, 0, 0], np.float32))
    # (row 0 carries state 1's weight to every state; the end is the FIRST of four equal states, state 0, which was entered
    # at row 0 from state 1 = s_1 with label 1, and kept by stay -- never by an equal advance -- afterwards)
    assert got["labels"] == [1] and got["path"] == [0] and abs(got["logp"] - 3 * math.log(0.25)) < 1e-12
