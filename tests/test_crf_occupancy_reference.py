"""CPU-only: the restatement of the CRF edge occupancies (tests/crf_occupancy_reference.py, the specification of
fcd_crf_occupancy_* in include/fcd.h) on tiny cases: occupancy64 against the enumeration of every alignment, its rows summing
to 1, every label's advance occupancies summing to 1 over the rows, occ = d crf_score / d ln p by central differences, and
occ - marg = d (score - logZ) / d x in the raw scores whose (p, init) crf_transitions_reference makes."""
import math

import numpy as np
import pytest

import crf_lattice_cases as CC
import crf_lattice_reference as R
import crf_marginals_reference as M
import crf_occupancy_reference as O
import crf_transitions_reference as TR


def tiny_cases():
    """(name, p (T, S, N) float32, init, y): T <= 6, S in {1, 3, 4, 5}; plain, with zeros, and with a sigma that leaves
    the table (a dead end: the labelling may be left without an alignment)"""
    rng = np.random.default_rng(31)
    out = []
    for S, N, T, L in ((4, 5, 1, 0), (4, 5, 1, 1), (4, 5, 5, 3), (4, 5, 6, 6), (4, 5, 6, 2), (1, 3, 4, 2), (1, 5, 5, 3),
                       (3, 2, 6, 3), (3, 2, 5, 0), (5, 4, 6, 3), (5, 4, 5, 2), (4, 3, 6, 4)):
        for flavour in ("plain", "zeros"):
            p = CC.posteriors(rng, 1, T, S, N)[0]
            if flavour == "zeros":
                p[rng.random(p.shape) < 0.15] = 0.0
            init = rng.random(S).astype(np.float32)
            if S == 1:
                y = [1] * L  # (any other label leaves the one-row table)
            elif S == 4 and N == 5 and L == 6:
                y = [2] * L  # a homopolymer: every state after the first shares sigma = 1
            else:
                y = [int(v) for v in rng.integers(1, N, L)]
            out.append(("S%d_N%d_T%d_L%d_%s" % (S, N, T, L, flavour), p, init, y))
    # sigma leaves the table: S = 5, N = 4 from sigma_0 = 4 by label 3 -> (4 * 3) mod 5 + 2 = 4; by label 3 from 3 -> 6
    p = CC.posteriors(rng, 1, 5, 5, 4)[0]
    out.append(("S5_N4_dead_end", p, np.array([0, 0, 0, 1, 0], np.float32), [3, 1]))
    out.append(("S1_N3_dead_end", CC.posteriors(rng, 1, 4, 1, 3)[0], np.ones(1, np.float32), [2, 1]))
    return out


TINY = tiny_cases()
IDS = [c[0] for c in TINY]


@pytest.mark.parametrize("name,p,init,y", TINY, ids=IDS)
def test_occupancy_by_enumeration(name, p, init, y):
    ref = O.occupancy64(p, init, y)
    want, adv, total = O.enumerate_occupancy(p, init, y)
    if want is None:
        assert ref["occ"] is None and not math.isfinite(ref["logp"])
        return
    assert abs(ref["logp"] - math.log(total)) <= 1e-12 * max(1.0, abs(ref["logp"]))
    assert np.abs(ref["occ"] - want).max() <= 1e-12, np.abs(ref["occ"] - want).max()
    assert np.abs(ref["adv"][:, :len(y)] - adv).max(initial=0.0) <= 1e-12
    # every row sums to 1; every label is emitted exactly once
    assert np.abs(ref["occ"].sum(axis=(1, 2)) - 1.0).max() <= 1e-12
    assert np.abs(ref["adv"][:, :len(y)].sum(axis=0) - 1.0).max(initial=0.0) <= 1e-12
    # the float32 arithmetic stays close to it
    r32 = O.occupancy32(p, init, y)
    assert r32["occ"].dtype == np.float32 and np.abs(r32["occ"] - ref["occ"]).max() <= 2e-6


def test_dead_ends_have_no_occupancy():
    for name, p, init, y in TINY[-2:]:
        assert O.occupancy64(p, init, y)["occ"] is None and R.crf_score(p, init, y) == -math.inf, name


@pytest.mark.parametrize("name,p,init,y", TINY, ids=IDS)
def test_occupancy_is_the_gradient_of_the_score_in_ln_p(name, p, init, y):
    """score(l) = ln sum over the alignments of exp(sum of l along the alignment), l = ln p.  The central difference with
    step h in one l[t][s][a] is occ + h^2 / 6 * score''' (xi): score is the cumulant generating function of the edge's
    indicator -- Bernoulli of probability occ, an edge being used at most once in an alignment -- so |score'''| =
    |m (1 - m) (1 - 2 m)| <= 0.0963, the truncation below 0.0963 h^2 / 6.  Scaling p by exp(+-h) costs one float64 rounding,
    and crf_score a handful per row on T <= 6 rows: each score within 16 units of 2^-53 max(1, |score|), which the difference
    divides by h.  The posteriors are float32 in crf_score's interface, so the steps are taken on a float64 copy through
    crf_score's own recurrence (R._rows' table lookup is exact).  h = 1e-4: the bound is about 1e-9."""
    ref = O.occupancy64(p, init, y)
    if ref["occ"] is None:
        return
    h = 1e-4
    bound = 0.0963 * h * h / 6 + 16 * 2.0 ** -53 * max(1.0, abs(ref["logp"])) / h
    assert bound < 2e-9
    worst = 0.0
    for idx in np.ndindex(*p.shape):
        if p[idx] == 0:
            assert ref["occ"][idx] == 0.0
            continue
        fd = (_score64(p, init, y, idx, math.exp(h)) - _score64(p, init, y, idx, math.exp(-h))) / (2 * h)
        worst = max(worst, abs(fd - ref["occ"][idx]))
    print("%s: largest |finite difference - occ| %.3g, bound %.3g" % (name, worst, bound))
    assert worst <= bound


def _score64(p, init, y, idx, factor):
    """crf_lattice_reference.crf_score's recurrence (band 0) with entry idx of p scaled by `factor` in float64"""
    T, S, N = p.shape
    L = len(y)
    q = p.astype(np.float64)
    q[idx] *= factor
    sig = R.trajectory(init, y, S, N)
    a = np.zeros(L + 1)
    a[0] = 1.0
    for t in range(T):
        n = np.zeros(L + 1)
        for k in range(L + 1):
            if 0 <= sig[k] < S:
                n[k] += a[k] * q[t, sig[k], 0]
            if k >= 1 and 0 <= sig[k - 1] < S:
                n[k] += a[k - 1] * q[t, sig[k - 1], y[k - 1]]
        a = n
    return math.log(a[L])


def test_score64_is_crf_score():
    for name, p, init, y in TINY:
        lp = R.crf_score(p, init, y)
        if math.isfinite(lp):
            assert abs(_score64(p, init, y, (0, 0, 0), 1.0) - lp) <= 1e-12 * max(1.0, abs(lp)), name


@pytest.mark.parametrize("S,N,T,y", [(4, 5, 6, [2, 1, 4]), (4, 5, 5, [3, 3, 3, 3]), (3, 2, 6, [1, 1]), (4, 3, 4, [])])
def test_occupancy_minus_marginals_is_the_gradient_of_the_loss(S, N, T, y):
    """raw scores x -> (p, init) = crf_transitions_reference.transitions64(x); with sigma_0 the first maximum of init,
    f(x) = ln(init[sigma_0] P(y | x)) = (sum over y's alignments from sigma_0 of exp(score)) - logZ, and its gradient is
    occ - marg.  Both halves are cumulant generating functions of a Bernoulli indicator, so the central difference's
    truncation is below 2 * 0.0963 h^2 / 6; the float64 roundings of f (two log-space recurrences on T <= 6 rows) are
    within 32 units of 2^-53 max(1, |f|, |logZ|), divided by h.  h = 1e-4: about 2e-9.  p is float32 in occupancy64's
    interface: rounding transitions64's p to float32 moves occ by up to (T + 1) 2^-24 relative (T factors along an
    alignment and P), which the comparison allows for on top."""
    rng = np.random.default_rng(100 + S + N + T)
    x = TR.random_scores(rng, T, S, N, sd=1.5).astype(np.float64)
    tr = TR.transitions64(x)
    init = tr["init"]
    s0 = R.trajectory(init.astype(np.float32), [], S, N)[0]
    ref = O.occupancy64(tr["probs"].astype(np.float32), init.astype(np.float32), y)
    marg = M.marginals64(x)["marg"]
    grad = ref["occ"] - marg
    # ln(init[sigma_0] P) = score_x(y) - logZ, to rounding
    f0 = _numerator64(x, s0, y) - M.logz64(x)
    assert abs(f0 - (ref["logp"] + math.log(init[s0]))) <= (T + 2) * 2.0 ** -24
    h = 1e-4
    bound = 2 * 0.0963 * h * h / 6 + 32 * 2.0 ** -53 * max(1.0, abs(f0), abs(M.logz64(x))) / h + (T + 1) * 2.0 ** -24
    worst = 0.0
    for idx in np.ndindex(*x.shape):
        up, dn = x.copy(), x.copy()
        up[idx] += h
        dn[idx] -= h
        fd = ((_numerator64(up, s0, y) - M.logz64(up)) - (_numerator64(dn, s0, y) - M.logz64(dn))) / (2 * h)
        worst = max(worst, abs(fd - grad[idx]))
    print("S%d N%d T%d: largest |finite difference - (occ - marg)| %.3g, bound %.3g" % (S, N, T, worst, bound))
    assert worst <= bound


def _numerator64(x, s0, y):
    """ln of the sum over the alignments of y from start state s0 of exp(score), float64 log space"""
    T, S, N = x.shape
    L = len(y)
    nb = N - 1
    sig = [s0]
    for v in y:
        sig.append((sig[-1] * nb) % S + v - 1)
    a = np.full(L + 1, -np.inf)
    a[0] = 0.0
    for t in range(T):
        n = np.full(L + 1, -np.inf)
        for k in range(L + 1):
            c = []
            if 0 <= sig[k] < S:
                c.append(a[k] + x[t, sig[k], 0])
            if k >= 1 and 0 <= sig[k - 1] < S:
                c.append(a[k - 1] + x[t, sig[k - 1], y[k - 1]])
            n[k] = np.logaddexp.reduce(c) if c else -np.inf
        a = n
    return float(a[L])
