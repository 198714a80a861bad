"""CPU-only checks of tests/ctc_score_reference.py, the float64 restatement the scoring kernel is held to: it equals
the sum over every alignment (brute force) for every labelling of tiny cases under both collapse_repeats values, it
equals -torch.nn.functional.ctc_loss, and it is tied to the reference's own search: with a beam wide enough that
nothing is pruned, the beam search's final probabilities (tests/nbest_reference.py, src/search.rs:159-301) are the
same sums, relative to the best entry."""
import itertools
import math

import numpy as np
import pytest

import ctc_score_reference as R


def _posteriors(rng, T, N):
    x = np.exp(rng.standard_normal((T, N)) * 1.5)
    return (x / x.sum(1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("collapse", [True, False])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_restatement_equals_enumeration(T, collapse):
    rng = np.random.default_rng(100 + T)
    p = _posteriors(rng, T, 3)
    table = R.enumerate_all(p, collapse)
    assert abs(sum(table.values()) - 1.0) < 1e-6
    n = 0
    for L in range(0, T + 2):  # (one label more than rows: no alignment)
        for y in itertools.product((1, 2), repeat=L):
            got = R.ctc_logp(p, y, collapse)
            want = table.get(y, 0.0)
            if want == 0.0:
                assert got == -math.inf, (y, got)
            else:
                assert abs(got - math.log(want)) <= 1e-12 * max(1.0, abs(math.log(want))), (y, got, math.log(want))
                n += 1
    assert n == len(table)


def test_band_is_a_lower_bound_that_reaches_the_exact_value():
    rng = np.random.default_rng(7)
    p = _posteriors(rng, 12, 4)
    y, path = [1, 3, 3, 2], [1, 4, 6, 9]
    exact = R.ctc_logp(p, y)
    prev = -math.inf
    for W in (1, 2, 3, 8):
        v = R.ctc_logp(p, y, band=W, path=path)
        assert prev <= v <= exact + 1e-12
        prev = v
    assert abs(prev - exact) < 1e-12  # 2 * (k + 8) covers every state


def test_edge_cases_of_the_definition():
    rng = np.random.default_rng(8)
    p = _posteriors(rng, 5, 3)
    assert abs(R.ctc_logp(p, []) - np.log(p[:, 0].astype(np.float64)).sum()) < 1e-12
    assert R.ctc_logp(p[:0], []) == 0.0
    assert R.ctc_logp(p[:0], [1]) == -math.inf
    assert R.ctc_logp(p, [1, 2, 1, 2, 1, 2]) == -math.inf
    assert R.ctc_logp(p, [1, 1, 1]) > -math.inf and R.ctc_logp(p[:4], [1, 1, 1]) == -math.inf  # repeats need a blank between
    assert R.ctc_logp(p[:4], [1, 1, 1], collapse_repeats=False) > -math.inf
    assert math.isnan(R.ctc_logp(p, [1, 3]))
    assert math.isnan(R.ctc_logp(p, [0]))
    q = p.copy()
    q[2, 0] = np.nan
    assert math.isnan(R.ctc_logp(q, [1]))
    # the drop option only removes what is far below the row maximum
    assert R.ctc_logp(p, [1, 2], drop=2.0 ** -160) == R.ctc_logp(p, [1, 2])
    assert R.ctc_logp(p, [1, 2], drop=0.5) < R.ctc_logp(p, [1, 2])


def test_equals_torch_ctc_loss():
    import torch
    rng = np.random.default_rng(9)
    for T, N, y in ((1, 3, [2]), (7, 5, [1, 1, 4]), (30, 6, [5, 4, 4, 3, 1, 2, 2, 1]), (12, 4, [])):
        p = _posteriors(rng, T, N)
        lp = torch.log(torch.from_numpy(p.astype(np.float64)))[:, None, :]
        loss = torch.nn.functional.ctc_loss(lp, torch.tensor([y], dtype=torch.long).reshape(1, len(y)),
                                            torch.tensor([T]), torch.tensor([len(y)]), blank=0, reduction="none")
        assert abs(R.ctc_logp(p, y) + float(loss[0])) < 1e-10, (T, N, y)


@pytest.mark.parametrize("collapse", [True, False])
@pytest.mark.parametrize("T", [1, 3, 6])
def test_unpruned_beam_search_ranks_by_the_same_sums(T, collapse):
    """src/search.rs:186-241 with nothing pruned: entry i's probability is P(y_i) / (a common factor), so
    score_i / score_0 = exp(logp_i - logp_0) to f32 accuracy."""
    import nbest_reference as NR
    rng = np.random.default_rng(200 + T)
    p = _posteriors(rng, T, 3)
    st, hyps = NR.beam_search(p, 4096, 0.0, collapse_repeats=collapse, stable=True)
    assert st == NR.OK and len(hyps) >= 2
    table = R.enumerate_all(p, collapse)
    assert len(hyps) == len(table)  # the whole final beam: every labelling that has an alignment
    logp = [R.ctc_logp(p, labels, collapse) for labels, _, _ in hyps]
    for (labels, _, score), lp in zip(hyps, logp):
        want = math.exp(lp - logp[0])
        assert abs(score / hyps[0][2] - want) <= 1e-4 * want, (labels, score, want)
