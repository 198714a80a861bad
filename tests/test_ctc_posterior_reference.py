"""CPU-only: the restatement tests/ctc_posterior_reference.py against brute force -- every variant labelling's probability
summed over every alignment of a tiny read -- and on a hand-made read where two bases are nearly tied at one position."""
import math

import numpy as np
import pytest

import ctc_posterior_reference as PR
import ctc_score_reference as R


@pytest.mark.parametrize("collapse", [True, False])
@pytest.mark.parametrize("T,N,y", [(4, 3, [1, 2]), (5, 3, [1, 1]), (6, 3, [2, 1, 1]), (6, 2, [1, 1, 1]), (3, 3, [2]), (5, 3, [1, 2, 2, 1])])
def test_sub_equals_enumeration(T, N, y, collapse):
    rng = np.random.default_rng(T * 10 + N)
    p = rng.random((T, N)) + 0.05
    p /= p.sum(-1, keepdims=True)
    every = R.enumerate_all(p, collapse)
    sub = np.exp(PR.ctc_sub_logp(p, y, collapse))
    for k in range(len(y)):
        for c in range(1, N):
            want = every.get(tuple(y[:k] + [c] + y[k + 1:]), 0.0)
            assert abs(sub[k, c - 1] - want) <= 1e-12 * max(want, 1e-300), (k, c, sub[k, c - 1], want)
    post, logp = PR.ctc_posterior(p, y, collapse)
    want_p = every.get(tuple(y), 0.0)
    if want_p > 0:
        assert abs(math.exp(logp) - want_p) <= 1e-12 * want_p
        assert np.allclose(post.sum(-1), 1.0, atol=1e-12)
    else:
        assert logp == -math.inf and np.isnan(post).all()


def test_a_near_tie_shows_in_conf_and_nowhere_else():
    """A C G T, one row per base between blanks; the row of G gives G 0.47 and T 0.46: ACGT and ACTT nearly tied"""
    eps = 1e-3
    rows = []
    for base in (1, 2, 3, 4):
        r = np.full(5, eps)
        r[base] = 1.0 - 4 * eps
        rows.append(r)
        b = np.full(5, eps)
        b[0] = 1.0 - 4 * eps
        rows.append(b)
    rows[4] = np.array([0.03, 0.02, 0.02, 0.47, 0.46])
    p = np.array(rows)
    y = [1, 2, 3, 4]
    post, logp = PR.ctc_posterior(p, y)
    conf = post[np.arange(4), np.array(y) - 1]
    assert math.isfinite(logp)
    assert abs(conf[2] - 0.5) < 0.03 and abs(post[2, 3] - 0.5) < 0.03
    assert all(conf[k] > 0.99 for k in (0, 1, 3))
