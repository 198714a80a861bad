"""CPU-only: the two float64 restatements of fcd_crf_edits_* (tests/crf_edits_reference.py) -- every variant rescored, and
the chain definition on dense arrays -- pinned to the sum over every alignment of every variant labelling, enumerated, on
tiny cases: T <= 6, L <= 4, S = 1 / 4 / 16 at N = 5 and 8 at N = 3 (histories of 1, 1, 2 and 3 labels), T_r = L (every
insertion has probability 0, a deletion several alignments), T_r = L + 1 (an insertion exactly one), L = 0 and 1, an init row
whose first maximum is not state 0, and at S = 1 labels that leave the table.  Then the bands: the chain restatement equals
the rescored one at band 0 and at band >= L, rises with the band in between and never exceeds the exact value."""
import math

import numpy as np
import pytest

import crf_edits_reference as ER
import crf_lattice_cases as CC
import crf_lattice_reference as R

SHAPES = [(1, 5), (4, 5), (16, 5), (8, 3)]


def close(a, b, what, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, a, b)
    assert np.array_equal(np.isneginf(a), np.isneginf(b)), (what, a, b)
    ok = np.isfinite(a)
    assert np.all(np.abs(a[ok] - b[ok]) <= tol * np.maximum(1.0, np.abs(b[ok]))), (what, a, b)


def tiny(S, N, T, L, seed):
    rng = np.random.default_rng(1000 * S + 100 * N + 10 * T + L + seed)
    p = CC.posteriors(rng, 1, T, S, N)[0]
    init = rng.random(S).astype(np.float32)
    if S > 1:
        init[S - 1] = 2.0  # the first maximum is not state 0
    y = [1] * L if S == 1 else [int(v) for v in rng.integers(1, N, L)]
    return p, init, y


@pytest.mark.parametrize("S,N", SHAPES)
@pytest.mark.parametrize("T,L", [(1, 0), (3, 0), (1, 1), (2, 1), (4, 1), (2, 2), (3, 2), (4, 4), (5, 4), (6, 4), (6, 3)])
def test_both_restatements_are_the_enumeration(S, N, T, L):
    p, init, y = tiny(S, N, T, L, 0)
    assert S == 1 or R.trajectory(init, y, S, N)[0] == S - 1
    de, ie, le = ER.enumerated(p, init, y)
    assert math.isfinite(le)
    for name, f in (("rescored", ER.rescored), ("chain", ER.chain)):
        d, i, lp = f(p, init, y)
        assert d.shape == (L,) and i.shape == (L + 1, N - 1)
        assert abs(lp - le) <= 1e-12 * max(1.0, abs(le)), name
        close(d, de, (name, "deletion"))
        close(i, ie, (name, "insertion"))
    if T == L:
        assert np.isneginf(ie).all() and (L < 2 or S == 1 or np.isfinite(de).all())
    if T == L + 1:
        assert S == 1 or np.isfinite(ie).all()


def test_labels_that_leave_the_table_at_s1():
    """S = 1: a label other than 1 leads outside the table -- a dead end unless it is the last label, emitted at the last row;
    deleting such a label brings the labelling back to life, inserting one kills it"""
    rng = np.random.default_rng(3)
    p = CC.posteriors(rng, 1, 6, 1, 5)[0]
    init = np.ones(1, np.float32)
    for y in ([1, 1, 3], [1, 2, 1], [2], [1, 1, 1, 4]):
        de, ie, le = ER.enumerated(p, init, y)
        for f in (ER.rescored, ER.chain):
            d, i, lp = f(p, init, y)
            if not math.isfinite(le):
                assert lp == le and np.isnan(d).all() and np.isnan(i).all()
                continue
            close(d, de, (y, "deletion"))
            close(i, ie, (y, "insertion"))
        if y == [1, 1, 3]:
            assert math.isfinite(le) and np.isneginf(ie[:3, 1:]).all() and np.isfinite(ie[:3, 0]).all()
            assert np.isneginf(ie[3]).all() and np.isfinite(de).all()  # (nothing can follow the label that left the table)
    de, _, le = ER.enumerated(p, init, [1, 2, 1])
    assert le == -math.inf and math.isfinite(de[1])  # (what the restatements return NaN for: P(y | x) = 0)


@pytest.mark.parametrize("S,N", SHAPES)
def test_bands(S, N):
    rng = np.random.default_rng(40 + S + N)
    T, L = 14, 8
    p = CC.posteriors(rng, 1, T, S, N)[0]
    init = rng.random(S).astype(np.float32)
    y = [1] * L if S == 1 else [int(v) for v in rng.integers(1, N, L)]
    path = np.sort(rng.choice(T, L, replace=False))
    dr, ir, lr = ER.rescored(p, init, y)
    d0, i0, l0 = ER.chain(p, init, y)
    close(d0, dr, "band 0 deletion")
    close(i0, ir, "band 0 insertion")
    prev = None
    for band in (1, 2, 4, L, L + 3):
        d, i, lp = ER.chain(p, init, y, band, path)
        if not math.isfinite(lp):
            assert np.isnan(d).all() and np.isnan(i).all()
            continue
        slack = 1e-12
        assert np.all(d <= dr + slack) and np.all(i <= ir + slack), band
        if prev is not None:
            assert np.all(d >= prev[0] - slack) and np.all(i >= prev[1] - slack), band
        prev = (d, i)
        if band >= L:
            assert abs(lp - lr) <= 1e-12 * abs(lr)
            close(d, dr, ("band", band, "deletion"))
            close(i, ir, ("band", band, "insertion"))
    assert prev is not None
