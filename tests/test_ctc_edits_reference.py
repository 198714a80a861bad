"""CPU-only: the two float64 restatements of tests/ctc_edits_reference.py against one another, against a brute-force sum
over every alignment, and the properties a band must have.  The kernels are held to these restatements by
tests/test_ctc_edits_emu.py and tests/test_gpu_ctc_edits.py."""
import math

import numpy as np

import ctc_edits_reference as ER
import ctc_score_cases as SC
import ctc_score_reference as R


def _close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    inf = np.isinf(b)
    assert np.array_equal(a[inf], b[inf]), (a, b)
    ok = ~inf & ~np.isnan(b)
    assert np.all(np.abs(a[ok] - b[ok]) <= tol), (a, b, np.abs(a[ok] - b[ok]).max())


def _random_case(rng, n_max=5, t_max=10, l_max=5):
    N = int(rng.integers(2, n_max + 1))
    T = int(rng.integers(1, t_max + 1))
    L = int(rng.integers(0, l_max + 1))
    x = SC.posteriors(rng, 1, T, N)[0]
    y = [int(v) for v in rng.integers(1, N, size=L)]
    if L >= 2 and rng.integers(2):  # repeated labels next to the edit
        k = int(rng.integers(L - 1))
        y[k + 1] = y[k]
    return x, y


def test_dense_equals_rescored_in_exact_mode():
    rng = np.random.default_rng(20)
    seen = {"L0": 0, "L1": 0, "L>T": 0, "repeat": 0}
    for n in range(300):
        x, y = _random_case(rng)
        for collapse in (True, False):
            d0, i0, lp0 = ER.ctc_edits_rescored(x, y, collapse)
            d1, i1, lp1 = ER.ctc_edits_dense(x, y, collapse)
            assert (lp0 == lp1) or abs(lp0 - lp1) <= 1e-9
            _close(d1, d0, 1e-9)
            _close(i1, i0, 1e-9)
        seen["L0"] += len(y) == 0
        seen["L1"] += len(y) == 1
        seen["L>T"] += len(y) > x.shape[0]
        seen["repeat"] += any(a == b for a, b in zip(y, y[1:]))
    assert all(v >= 5 for v in seen.values()), seen


def test_against_the_sum_over_every_alignment():
    rng = np.random.default_rng(21)
    for n in range(30):
        x, y = _random_case(rng, n_max=3, t_max=6, l_max=4)
        for collapse in (True, False):
            every = R.enumerate_all(x, collapse)
            for fn in (ER.ctc_edits_rescored, ER.ctc_edits_dense):
                d, i, lp = fn(x, y, collapse)
                if not math.isfinite(lp):
                    assert np.isnan(d).all() and np.isnan(i).all()
                    continue
                P = math.exp(lp)
                for k in range(len(y)):
                    want = every.get(tuple(y[:k] + y[k + 1:]), 0.0)
                    assert abs(math.exp(d[k]) * P - want) <= 1e-12 + 1e-9 * want, (fn.__name__, y, k)
                for g in range(len(y) + 1):
                    for c in range(1, x.shape[1]):
                        want = every.get(tuple(y[:g] + [c] + y[g:]), 0.0)
                        assert abs(math.exp(i[g, c - 1]) * P - want) <= 1e-12 + 1e-9 * want, (fn.__name__, y, g, c)


def test_band_is_a_lower_bound_that_rises_to_the_exact_value():
    rng = np.random.default_rng(22)
    for n in range(40):
        N, T = int(rng.integers(2, 6)), int(rng.integers(4, 25))
        L = int(rng.integers(1, max(2, T // 2)))
        x = SC.posteriors(rng, 1, T, N)[0]
        y = [int(v) for v in rng.integers(1, N, size=L)]
        path = sorted(int(v) for v in rng.choice(T, size=L, replace=False))
        collapse = bool(n & 1)
        exact = ER.ctc_edits_rescored(x, y, collapse)
        if not math.isfinite(exact[2]):
            continue
        prev = None
        for W in (1, 2, 4, L + 1, L + 7):
            d, i, lp = ER.ctc_edits_dense(x, y, collapse, W, path)
            if not math.isfinite(lp):  # nothing of y inside so narrow a window
                assert prev is None
                continue
            # as probabilities: exp(ratio) * P(y inside the window)
            cur = (d + lp, i + lp)
            for got, ex in zip(cur, (exact[0] + exact[2], exact[1] + exact[2])):
                assert np.all(got <= ex + 1e-9), (y, W)
            if prev is not None:
                for lo_v, hi_v in zip(prev, cur):
                    assert np.all(lo_v <= hi_v + 1e-9), (y, W)
            if W > L:
                _close(d, exact[0], 1e-9)
                _close(i, exact[1], 1e-9)
            prev = cur


def test_case_table_ties_are_rare():
    """EditResult.best is compared with the restatement's argmax wherever the two best edits are further apart than twice
    the tolerance: the table must leave at most one labelling in ten out."""
    import ctc_edits_cases as EC
    import fast_ctc_decode_amd as fcd
    from emu_util import emulated_kernels
    with emulated_kernels():
        total = close = 0
        for case in EC.CASES:
            c = EC.build_case(fcd, case)
            for band in c["bands"]:
                t, k = EC.tie_share(c, band)
                total += t
                close += k
    print("ctc_edits: %d of %d labellings have their two best edits within twice the tolerance" % (close, total))
    assert total > 0 and close * 10 <= total
