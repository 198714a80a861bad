"""CPU-only: the float64 restatement tests/crf_posterior_reference.py pinned against the brute-force enumeration of every
alignment of every variant (crf_lattice_reference.enumerate_alignments) on tiny cases -- T <= 6, L <= 3, S = 1, 4, 16 at
N = 5 and S = 8 at N = 3 -- and the identity sub[k][y_k] = P(y | x).  Also: fast_ctc_decode_amd exports the entry points the
restatement specifies."""
import itertools
import math

import numpy as np
import pytest

import crf_lattice_reference as R
import crf_posterior_reference as PR


def _posteriors(rng, T, S, N):
    x = rng.random((T, S, N)) ** 2
    return (x / x.sum(-1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("S,N", [(1, 5), (4, 5), (16, 5), (8, 3)])
def test_restatement_against_enumeration(S, N):
    rng = np.random.default_rng(100 + S + N)
    n = 0
    for T, L in itertools.product((1, 3, 6), (1, 2, 3)):
        if L > T:
            continue
        x = _posteriors(rng, T, S, N)
        init = rng.random(S).astype(np.float32)
        y = [int(v) for v in rng.integers(1, N, L)]
        if S == 1:  # (sigma_{k+1} = y_k - 1: any label but 1 leaves the one-row table, a dead end unless entered last)
            y = [1] * (L - 1) + y[-1:]
        post, logp = PR.crf_posterior(x, init, y)
        sub, _ = PR.crf_substitutions(x, init, y)
        total = sum(w for w, _ in R.enumerate_alignments(x, init, y))
        assert abs(logp - math.log(total)) <= 1e-12 * max(1.0, abs(math.log(total)))
        for k in range(L):
            brute = [sum(w for w, _ in R.enumerate_alignments(x, init, y[:k] + [c] + y[k + 1:])) for c in range(1, N)]
            assert sub[k, y[k] - 1] == logp  # the called label's variant is the labelling itself
            assert abs(brute[y[k] - 1] - total) <= 1e-15 * total
            want = np.array(brute) / sum(brute)
            assert (S == 1 and k < L - 1) == (0.0 in brute)  # (S = 1: a variant that leaves the table before the end has none)
            assert np.all(np.abs(post[k] - want) <= 1e-12 * want + 1e-300), (S, N, T, L, k, post[k], want)
            assert abs(post[k].sum() - 1.0) <= 1e-12
            n += 1
    assert n >= 10


def test_rows_without_a_value():
    rng = np.random.default_rng(3)
    x = _posteriors(rng, 4, 4, 5)
    init = np.array([0.1, 0.9, 0.2, 0.3], np.float32)
    post, logp = PR.crf_posterior(x, init, [1, 2, 3, 4, 1])  # L > T
    assert logp == -math.inf and post.shape == (5, 4) and np.isnan(post).all()
    post, logp = PR.crf_posterior(x, init, [1, 5])  # a bad label
    assert math.isnan(logp) and np.isnan(post).all()
    post, logp = PR.crf_posterior(x, init, [])
    assert post.shape == (0, 4) and math.isfinite(logp)
    # a NaN only a variant reads: sigma of y = 1, 2 (after label 3), 0 (after label 1); the variant [4, 1] stays in model
    # state 3 over row 1; state 2 is not live at row 0, so no variant of position 1 stays in it over row 1
    xn = x.copy()
    xn[1, 3, 0] = np.nan
    assert R.trajectory(init, [3, 1], 4, 5) == [1, 2, 8 % 4 + 0]
    post, logp = PR.crf_posterior(xn, init, [3, 1])
    assert math.isfinite(logp) and np.isnan(post[0]).all() and np.isfinite(post[1]).all()


def test_the_package_exports_the_entry_points():
    import fast_ctc_decode_amd as fcd
    assert callable(fcd.crf_posterior) and callable(fcd.crf_posterior_batch_raw)
