"""CPU-only checks of tests/ctc_align_reference.py, the restatement the alignment kernels are held to exactly: on every
labelling of tiny cases (T <= 7, L <= 3, N <= 3, both collapse_repeats values) its alignment is the float64 enumeration's
best one wherever the two best differ by more than 1e-4 relative, and its logp agrees within 2 T 2^-24 (one f32 rounding
per row)."""
import itertools
import math

import numpy as np
import pytest

import ctc_align_reference as A


def _posteriors(rng, T, N):
    x = rng.random((T, N)) ** 3 + 1e-3
    return (x / x.sum(-1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("collapse", [True, False])
def test_against_enumeration(collapse):
    rng = np.random.default_rng(11 + collapse)
    checked = decided = 0
    for T, N in ((1, 2), (2, 3), (4, 2), (5, 3), (7, 3), (7, 2), (3, 3), (6, 3), (7, 3), (6, 2), (4, 3), (7, 3)):
        p = _posteriors(rng, T, N)
        for L in range(0, 4):
            for y in itertools.product(range(1, N), repeat=L):
                got = A.ctc_align(p, y, collapse)
                alns = A.enumerate_alignments(p, y, collapse)
                if not alns:
                    assert got["logp"] == -math.inf and got["states"] is None, (T, N, y)
                    continue
                checked += 1
                assert abs(got["logp"] - math.log(alns[0][0])) <= 2 * T * 2.0 ** -24, (T, N, y)
                if len(alns) == 1 or alns[1][0] < alns[0][0] * (1 - 1e-4):
                    decided += 1
                    assert tuple(got["states"]) == alns[0][1], (T, N, y, got["states"], alns[0], alns[1:2])
                start, count = A.spans(got["states"], L)  # (spans() is independent of the walk that fills start / count)
                assert got["start"] == start and got["count"] == count
                assert all(c >= 1 for c in got["count"]) and (collapse or all(c == 1 for c in got["count"]))
    assert checked > 100 and decided > 0.9 * checked


def test_tie_rule_and_edges():
    # every posterior 0.5: all alignments tie.  State 2L beats 2L-1 at the end, and walking back a cell stays where it
    # is as long as staying was possible: the label is taken as early as it can be
    p = np.full((4, 2), 0.5, np.float32)
    got = A.ctc_align(p, [1], True)
    assert got["states"] == [1, 2, 2, 2] and got["start"] == [0] and got["count"] == [1]
    got = A.ctc_align(p, [1, 1], True)  # label, blank, label
    assert got["states"] == [1, 2, 3, 4] and got["start"] == [0, 2]
    got = A.ctc_align(p, [1, 1], False)  # every label row emits: no blank needed between the two
    assert got["states"] == [1, 3, 4, 4] and got["count"] == [1, 1]
    assert A.ctc_align(p, [1, 1, 1], True)["logp"] == -math.inf  # five rows needed
    assert A.ctc_align(p, [1, 1, 1], False)["logp"] == pytest.approx(4 * math.log(0.5))
    assert math.isnan(A.ctc_align(p, [2], True)["logp"]) and math.isnan(A.ctc_align(p, [0], True)["logp"])
    assert A.ctc_align(p[:0], [], True)["logp"] == 0.0 and A.ctc_align(p[:0], [1], True)["logp"] == -math.inf
    assert A.ctc_align(p, [], True)["logp"] == pytest.approx(4 * math.log(0.5))
    for bad in (np.nan, np.inf, -0.25):
        q = p.copy()
        q[3, 0] = bad
        assert math.isnan(A.ctc_align(q, [1], True)["logp"])
    assert A.ctc_align(p[:1], [1, 1], True)["logp"] == -math.inf  # L > T comes before the posterior test
    # the exponent is unbounded: 300 rows of 2^-100 neither underflow nor change the alignment
    tiny = np.full((300, 2), np.float32(2.0 ** -100), np.float32)
    got = A.ctc_align(tiny, [1], True)
    assert got["logp"] == pytest.approx(-300 * 100 * math.log(2.0)) and got["count"] == [1]
    # a band around a late path still holds state 0 .. 2 of a one-label labelling: an alignment exists
    p8 = np.full((8, 2), 0.5, np.float32)
    assert A.ctc_align(p8, [1], True, band=1, path=[7])["logp"] == pytest.approx(8 * math.log(0.5))
    # a band that keeps the end out of reach: k(t) = 0 on every row, so band 1 ends at state 2 of 11 -- no alignment
    p40 = np.full((40, 3), 0.25, np.float32)
    far = A.ctc_align(p40, [1, 2, 1, 2, 1], True, band=1, path=[40] * 5)
    assert far["logp"] == -math.inf and far["states"] is None and far["count"] is None
    assert A.ctc_align(p40, [1, 2, 1, 2, 1], True, band=5, path=[40] * 5)["logp"] > -math.inf  # 2 (0 + 5) = 10: reaches 2L
    # qualities: f32 sum in row order, then one division
    x = np.array([[0.1, 0.9], [0.3, 0.7], [0.2, 0.8], [0.9, 0.1]], np.float32)
    got = A.ctc_align(x, [1], True)
    assert got["start"] == [0] and got["count"] == [3]
    assert got["qual"][0] == np.float32(np.float32(np.float32(x[0, 1] + x[1, 1]) + x[2, 1]) / np.float32(3))
