"""CPU-only: the restatements of the CRF edge marginals (tests/crf_marginals_reference.py, the specification of
fcd_crf_marginals_* in include/fcd.h) on tiny cases: marginals64 against the enumeration of every start state and symbol
sequence, its rows summing to 1, its state sums being the occupancy exp(alpha + beta - logZ), marg = d logZ / d x by central
differences of the float64 logZ, and the float32 arithmetic's distance to it on the table the kernel is checked on."""
import numpy as np
import pytest

import crf_marginals_cases as MC
import crf_marginals_reference as M
import crf_transitions_reference as R


def tiny_cases():
    rng = np.random.default_rng(23)
    shapes = [(4, 5, T) for T in (1, 2, 3, 4)] + [(3, 2, T) for T in (1, 2, 3, 4, 5, 6)] + [(4, 3, 3), (8, 3, 3)]
    out = []
    for S, N, T in shapes:
        for flavour in ("plain", "neg_inf"):
            x = R.random_scores(rng, T, S, N, sd=2.0, n_neg_inf=0 if flavour == "plain" else max(1, S * N * T // 6))
            out.append(("S%d_N%d_T%d_%s" % (S, N, T, flavour), x))
    return out


TINY = tiny_cases()
IDS = [c[0] for c in TINY]


@pytest.mark.parametrize("name,x", TINY, ids=IDS)
def test_marginals_by_enumeration(name, x):
    ref = M.marginals64(x)
    assert ref["ok"]
    want, logz = M.enumerate_marginals(x)
    assert np.abs(ref["marg"] - want).max() <= 1e-12, np.abs(ref["marg"] - want).max()
    assert abs(ref["logz"] - logz) <= 1e-12
    assert (ref["marg"][np.isneginf(x)] == 0).all()


@pytest.mark.parametrize("name,x", TINY, ids=IDS)
def test_rows_sum_to_one_and_states_to_their_occupancy(name, x):
    ref = M.marginals64(x)
    assert np.abs(ref["marg"].sum(axis=(1, 2)) - 1.0).max() <= 1e-12
    assert np.abs(ref["emit"].sum(axis=1) - 1.0).max() <= 1e-12
    T = x.shape[0]
    occ = np.exp(ref["alpha"][:T] + ref["beta"][:T] - ref["logz"])
    assert np.abs(ref["marg"].sum(axis=2) - occ).max() <= 1e-12
    # logZ and the failure rule are crf_transitions_reference's
    tr = R.transitions64(x)
    assert abs(tr["logz"] - ref["logz"]) <= 1e-12


@pytest.mark.parametrize("name,x", TINY, ids=IDS)
def test_marginals_are_the_gradient_of_logz(name, x):
    """Central difference with step h: (logZ(x + h e) - logZ(x - h e)) / 2h = marg + h^2 / 6 * logZ''' (xi).  logZ is the
    cumulant generating function of the edge's indicator, a Bernoulli variable of probability m, so logZ''' = m (1 - m)
    (1 - 2 m), at most 1 / (6 sqrt 3) < 0.0963 in magnitude: the truncation is below 0.0963 h^2 / 6.  Each logZ carries a
    rounding error of at most 16 units of 2^-53 max(1, |logZ|) (a handful of float64 operations per row on T <= 6 rows), which
    the difference divides by h.  h = 1e-4 makes the two about equal: the bound is their sum, about 1e-9."""
    h = 1e-4
    ref = M.marginals64(x)
    bound = 0.0963 * h * h / 6 + 16 * 2.0 ** -53 * max(1.0, abs(ref["logz"])) / h
    assert bound < 2e-9
    x64 = x.astype(np.float64)
    worst = 0.0
    for idx in np.ndindex(*x.shape):
        if np.isneginf(x64[idx]):
            assert ref["marg"][idx] == 0.0  # (a forbidden transition stays forbidden under any finite step)
            continue
        up, dn = x64.copy(), x64.copy()
        up[idx] += h
        dn[idx] -= h
        fd = (M.logz64(up) - M.logz64(dn)) / ((x64[idx] + h) - (x64[idx] - h))
        worst = max(worst, abs(fd - ref["marg"][idx]))
    print("%s: largest |finite difference - marg| %.3g, bound %.3g" % (name, worst, bound))
    assert worst <= bound


def test_failures_and_the_empty_read():
    rng = np.random.default_rng(4)
    x = R.random_scores(rng, 4, 4, 3)
    y = x.copy()
    y[2] = -np.inf  # a row nothing passes
    assert not M.marginals64(y)["ok"] and not M.marginals32(y)["ok"]
    for v in (np.nan, np.inf):
        y = x.copy()
        y[1, 2, 1] = v
        assert not M.marginals64(y)["ok"] and not M.marginals32(y)["ok"]
    for fn in (M.marginals64, M.marginals32):
        e = fn(np.zeros((0, 6, 3), np.float32))
        assert e["ok"] and e["logz"] == np.log(6.0) and e["marg"].shape == (0, 6, 3) and e["emit"].shape == (0, 3)


@pytest.mark.parametrize("name,x", TINY, ids=IDS)
def test_float32_restatement_on_tiny_cases(name, x):
    ref, r32 = M.marginals64(x), M.marginals32(x)
    assert r32["ok"] and r32["marg"].dtype == np.float32
    assert np.abs(r32["marg"] - ref["marg"]).max() <= 2e-6 and np.abs(r32["emit"] - ref["emit"]).max() <= 2e-6
    assert (r32["marg"][np.isneginf(x)] == 0).all()


@pytest.mark.parametrize("case", MC.CASES, ids=[c["name"] for c in MC.CASES])
def test_float32_restatement_on_the_table(case):
    """err32 per case (the unit of the kernel's allowance)"""
    c = MC.build_case(case)
    for b in range(c["B"]):
        assert c["mrefs"][b]["ok"] and c["mrefs32"][b]["ok"]
    print("%s: err32 = %.3g" % (c["name"], c["merr32"]))
    assert c["merr32"] < (1e-3 if c.get("shift") else 2e-5)
