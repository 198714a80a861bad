"""CPU-only, no kernels: the restatement tests/crf_lattice_reference.py pinned three ways -- against the enumeration of
every C(T, L) alignment of tiny cases, against the unpruned CRF beam search of tests/nbest_reference.py (score differences
between the hypotheses of a read equal the differences of the beam's final ln-probabilities), and on every edge case of the
definition in include/fcd.h."""
import itertools
import math

import numpy as np
import pytest

import crf_lattice_reference as R
import nbest_reference as NB
from crf_lattice_cases import posteriors

SHAPES = [(4, 5), (16, 5), (6, 3), (3, 2), (5, 4)]


def _labellings(N, max_len):
    for L in range(max_len + 1):
        yield from itertools.product(range(1, N), repeat=L)


@pytest.mark.parametrize("S,N", SHAPES)
def test_enumeration(S, N):
    """the sum over every alignment is the score; the best of them is the alignment"""
    rng = np.random.default_rng(100 * S + N)
    for T in (1, 2, 5, 8):
        x = posteriors(rng, 1, T, S, N)[0]
        init = rng.random(S + (1 if (S, N) == (5, 4) else 0)).astype(np.float32)
        ys = list(_labellings(N, min(4, T)))
        for y in (ys if len(ys) <= 40 else [ys[j] for j in rng.choice(len(ys), 40, replace=False)]):
            al = R.enumerate_alignments(x, init, y)
            assert len(al) == math.comb(T, len(y))
            total = sum(w for w, _ in al)
            score = R.crf_score(x, init, y)
            got = R.crf_align(x, init, y)
            if total == 0.0:  # (a state outside the table on every alignment)
                assert score == -math.inf and got["logp"] == -math.inf and got["start"] is None
                continue
            assert abs(score - math.log(total)) <= 1e-12 * max(1.0, abs(score)), (T, y)
            best = max(w for w, _ in al)
            assert abs(got["logp"] - math.log(best)) <= 2 * T * 2.0 ** -24, (T, y)
            rows = tuple(got["start"])
            w_rows = dict((r, w) for w, r in al)[rows]
            assert abs(math.log(w_rows) - math.log(best)) <= 4 * T * 2.0 ** -24, (T, y)
            second = sorted((w for w, _ in al), reverse=True)[1] if len(al) > 1 else 0.0
            if second < best * (1 - 8 * T * 2.0 ** -24):  # a best alignment no rounding can unseat
                assert rows == max(al)[1], (T, y)
    assert (S, N) != (5, 4) or any(not 0 <= s < S for s in R.trajectory(np.ones(6, np.float32), [3, 3, 3], S, N))


@pytest.mark.parametrize("S,N", SHAPES)
def test_tie_rule(S, N):
    """posteriors that are powers of two: every product is exact in f32 and in float64, ties are exact, and the stay
    candidate is kept unless the advance is strictly greater -- walking back from the last row, every label is emitted as
    EARLY as a best alignment allows, the last label first"""
    rng = np.random.default_rng(7 * S + N)
    for T in (3, 6, 8):
        x = (2.0 ** -rng.integers(1, 3, (T, S, N))).astype(np.float32)
        init = rng.random(S).astype(np.float32)
        for y in list(_labellings(N, min(3, T)))[:30]:
            al = R.enumerate_alignments(x, init, y)
            best = max(w for w, _ in al)
            if best == 0.0:
                continue
            want = min((r for w, r in al if w == best), key=lambda r: r[::-1])
            got = R.crf_align(x, init, y)
            assert tuple(got["start"]) == want and got["logp"] == math.log(best), (T, y)
    x = np.full((5, S, N), 0.5, np.float32)
    if S >= N - 1 and (S, N) != (5, 4):
        assert R.crf_align(x, np.ones(S, np.float32), [1, 1])["start"] == [0, 1]


@pytest.mark.parametrize("S,N", [(4, 5), (16, 5), (3, 2), (6, 3), (5, 4)])
def test_unpruned_beam(S, N):
    """a beam wider than the number of labellings, threshold 0: for all hypotheses i, j of a read, score_i - score_j
    equals ln p_i - ln p_j of the beam's final probabilities, within 16 T 2^-24 (about four f32 roundings per step on
    each side, doubled)"""
    T, reads = 7, 6
    rng = np.random.default_rng(31 * S + N)
    nb = N - 1
    width = sum(nb ** L for L in range(T + 1)) + 1
    skipped = compared = 0
    for _ in range(reads):
        x = posteriors(rng, 1, T, S, N)[0]
        init = rng.random(S).astype(np.float32)
        st, hyps = NB.crf_beam_search(x, init, min(width, 4000), 0.0, stable=True)
        if st != NB.OK:
            skipped += 1
            continue
        hyps = [h for h in hyps if h[2] > 0][:150]
        sc = [R.crf_score(x, init, h[0]) for h in hyps]
        lp = [math.log(float(h[2])) for h in hyps]
        for i in range(len(hyps)):
            for j in (0, len(hyps) // 2, len(hyps) - 1):
                assert abs((sc[i] - sc[j]) - (lp[i] - lp[j])) <= 16 * T * 2.0 ** -24, (i, j, sc[i], sc[j], lp[i], lp[j])
                compared += 1
    if (S, N) in ((4, 5), (16, 5)):  # S a power of nb: the trajectory never leaves the table
        assert 4 * skipped < reads
    assert compared or skipped == reads


def test_edge_cases():
    rng = np.random.default_rng(3)
    x = posteriors(rng, 1, 6, 4, 5)[0]
    init = np.array([0.1, 0.7, 0.7, 0.2], np.float32)
    assert R.trajectory(init, [2, 4], 4, 5) == [1, (1 * 4) % 4 + 1, (1 * 4) % 4 + 3]  # the FIRST maximum
    assert R.trajectory(np.array([np.nan, -1.0], np.float32), [], 4, 5) == [1]
    for f in (R.crf_score, lambda *a: R.crf_align(*a)["logp"]):
        assert math.isnan(f(x, init, [1, 5])) and math.isnan(f(x, init, [0]))
        assert f(x[:0], init, []) == 0.0 and f(x[:0], init, [1]) == -math.inf
        assert f(x, init, [1] * 7) == -math.inf
        assert abs(f(x, init, []) - np.log(x[:, 1, 0].astype(np.float64)).sum()) <= 6 * 2.0 ** -24
    # L = T_r: every row emits, one alignment
    y = [1, 2, 3, 4, 1, 2]
    one = R.crf_align(x, init, y)
    assert one["start"] == list(range(6)) and abs(one["logp"] - R.crf_score(x, init, y)) <= 6 * 2.0 ** -24
    # a NaN in a contributing cell / among the values a live cell reads; elsewhere it is never read
    bad = x.copy()
    sig = R.trajectory(init, [1, 2], 4, 5)
    bad[2, sig[1], 0] = np.nan
    assert math.isnan(R.crf_score(bad, init, [1, 2])) and math.isnan(R.crf_align(bad, init, [1, 2])["logp"])
    other = x.copy()
    other[2, [s for s in range(4) if s not in sig][0], :] = np.nan
    assert R.crf_score(other, init, [1, 2]) == R.crf_score(x, init, [1, 2])
    assert R.crf_align(other, init, [1, 2])["start"] == R.crf_align(x, init, [1, 2])["start"]
    for v in (np.inf, -0.5):
        neg = x.copy()
        neg[0, sig[0], 1] = v
        assert math.isnan(R.crf_align(neg, init, [1, 2])["logp"])
    # rows the window cannot use are not read: state 0 cannot be held past row T - 1 - L
    late = x.copy()
    assert R.trajectory(init, [3, 1], 4, 5) == [1, 2, 0]
    late[5, 1, 0] = np.nan
    assert math.isfinite(R.crf_score(late, init, [3, 1])) and R.crf_align(late, init, [3, 1])["start"] is not None
    # a state outside the table (S = 5, N = 4): reads as 0 -- a dead end, except as the state entered at the last row
    x5 = posteriors(rng, 1, 3, 5, 4)[0]
    i5 = np.array([0, 0, 0, 0, 1], np.float32)
    assert R.trajectory(i5, [3], 5, 4) == [4, 4]
    assert R.trajectory(i5, [3, 3, 3], 5, 4)[2:] == [4, 4]
    i6 = np.array([0, 0, 0, 1, 0], np.float32)
    assert R.trajectory(i6, [3], 5, 4) == [3, 6]
    assert R.crf_align(x5, i6, [3])["start"] == [2] and math.isfinite(R.crf_score(x5, i6, [3]))  # entered at the last row
    assert R.crf_score(x5, i6, [3, 1]) == -math.inf and R.crf_align(x5, i6, [3, 1])["logp"] == -math.inf
    # the band: a window that holds everything is the exact lattice; a narrow one is a lower bound; one that never
    # reaches the last state has no alignment
    xl = posteriors(rng, 1, 40, 4, 5)[0]
    yl = [1, 2, 3] * 5
    pth = list(range(2, 32, 2))
    ex = R.crf_score(xl, init, yl)
    assert R.crf_score(xl, init, yl, 64, pth) == ex and R.crf_align(xl, init, yl, 64, pth) == R.crf_align(xl, init, yl)
    s1, s2 = R.crf_score(xl, init, yl, 1, pth), R.crf_score(xl, init, yl, 2, pth)
    a1, a2 = R.crf_align(xl, init, yl, 1, pth)["logp"], R.crf_align(xl, init, yl, 2, pth)["logp"]
    assert s1 <= s2 <= ex and a1 <= a2 <= R.crf_align(xl, init, yl)["logp"] and a1 <= s1
    far = [0] * 15  # k(t) = 15 from row 0 on: band 1 holds states 14 .. 15, which no alignment has reached by then
    assert R.crf_score(xl, init, yl, 1, far) == -math.inf and R.crf_align(xl, init, yl, 1, far)["logp"] == -math.inf
