"""TEST INFRASTRUCTURE: what fcd_crf_occupancy_* computes (include/fcd.h), restated in numpy -- the specification the walk
(csrc/crf_posterior.hip, crfp_occ_walk) is held to.

Everything is crf_lattice_reference's: the trajectory sigma_k, P(t, k, j) = p[t][sigma_k][j] (0 outside the table), the states
k = 0 .. L, the window of a row.  With alpha_{-1} = [k = 0], alpha_t[k] = alpha_{t-1}[k] P(t,k,0) + alpha_{t-1}[k-1] P(t,k-1,y_{k-1}),
beta_{T-1} = [k = L], beta_{u-1}[k] = P(u,k,0) beta_u[k] + P(u,k,y_k) beta_u[k+1] (a value enters a cell only where both its
source and the cell are live in their rows' windows) and P = alpha_{T-1}[L]:

    stay_t[k] = alpha_{t-1}[k] P(t,k,0)   beta_t[k]   / P
    adv_t[k]  = alpha_{t-1}[k] P(t,k,y_k) beta_t[k+1] / P              (k < L)
    occ[t][s][0] = sum_{k: sigma_k = s} stay_t[k]      occ[t][s][a] = sum_{k: sigma_k = s, y_k = a} adv_t[k]

  occupancy64   the definition in float64 (rows rescaled by exact powers of two): the reference of every check
  occupancy32   the stated ARITHMETIC in float32: every product and every sum rounded to float32 once, the rows rescaled by
                exact powers of two (f32 with an unbounded exponent), a term = ((alpha * p) * beta) scaled exactly, then
                divided by P's mantissa; the terms of an entry added in ascending k.  Its distance to occupancy64 is the
                unit of crf_ctc_loss's allowance (tests/test_gpu_crf_occupancy.py)
  enumerate_occupancy   the same by the enumeration of every alignment of a tiny case

Each returns dict(occ (T, S, N) or None, stay (T, L + 1), adv (T, L + 1), logp); occ is None whenever P(y | x) is not a
positive finite number (logp says which: crf_lattice_reference.crf_score's value)."""
import math

import numpy as np

import crf_lattice_reference as R


def _norm(v):
    """(v / 2^e, e) with the largest positive finite entry of v in [0.5, 1); e = 0 where there is none"""
    good = v[np.isfinite(v) & (v > 0)]
    if not good.size:
        return v, 0
    e = int(np.frexp(good.max())[1])
    return np.ldexp(v, -e), e


def _occupancy(p, init, y, band, path, f):
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.ndim == 3
    T, S, N = p.shape
    y = [int(v) for v in y]
    L = len(y)
    logp = R.crf_score(p, init, y, band, path)
    none = dict(occ=None, stay=None, adv=None, logp=logp)
    if not math.isfinite(logp) or T == 0:
        return none
    path = [int(v) for v in path] if band else None
    sig = R.trajectory(init, y, S, N)
    p0, py = R._rows(p, sig, y)
    p0, py = p0.astype(f), py.astype(f)
    win = [(0, 0)] + [R.window(t, T, L, band, path) for t in range(T)]  # win[t + 1]: row t; win[0]: "row -1"
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        # alpha[t + 1]: row t, scaled by 2^-ea[t + 1]
        alpha, ea = [np.zeros(L + 1, f)], [0]
        alpha[0][0] = 1
        for t in range(T):
            a, (plo, phi), (lo, hi) = alpha[-1], win[t], win[t + 1]
            n = np.zeros(L + 1, f)
            for k in range(lo, hi + 1):
                c0 = a[k] * p0[t, k] if plo <= k <= phi else f(0)
                c1 = a[k - 1] * py[t, k - 1] if k >= 1 and plo <= k - 1 <= phi else f(0)
                n[k] = f(c0) + f(c1)
            n, e = _norm(n)
            alpha.append(n)
            ea.append(ea[-1] + e)
        # beta[t]: row t, scaled by 2^-eb[t]
        beta, eb = [None] * T, [0] * T
        b = np.zeros(L + 1, f)
        lo, hi = win[T]
        if lo <= L <= hi:
            b[L] = 1
        beta[T - 1] = b
        for u in range(T - 1, 0, -1):
            (lo, hi), (plo, phi) = win[u + 1], win[u]  # row u (the values read), row u - 1 (the cells written)
            n = np.zeros(L + 1, f)
            for s in range(plo, phi + 1):
                c0 = p0[u, s] * b[s] if lo <= s <= hi else f(0)
                c1 = py[u, s] * b[s + 1] if s < L and lo <= s + 1 <= hi else f(0)
                n[s] = f(c0) + f(c1)
            b, e = _norm(n)
            beta[u - 1] = b
            eb[u - 1] = eb[u] + e
        pm, pe = np.frexp(alpha[T][L])
        pm, pe = f(pm), int(pe) + ea[T]
        if not pm > 0:
            return none
        stay, adv = np.zeros((T, L + 1), f), np.zeros((T, L + 1), f)
        occ = np.zeros((T, S, N), f)
        for t in range(T):
            a, b, (plo, phi), (lo, hi) = alpha[t], beta[t], win[t], win[t + 1]
            x = ea[t] + eb[t] - pe
            for k in range(plo, phi + 1):
                if lo <= k <= hi:
                    stay[t, k] = f(np.ldexp(f(f(a[k] * p0[t, k]) * b[k]), x)) / pm
                if k < L and lo <= k + 1 <= hi:
                    adv[t, k] = f(np.ldexp(f(f(a[k] * py[t, k]) * b[k + 1]), x)) / pm
                if 0 <= sig[k] < S:
                    occ[t, sig[k], 0] = f(occ[t, sig[k], 0] + stay[t, k])
                    if k < L:
                        occ[t, sig[k], y[k]] = f(occ[t, sig[k], y[k]] + adv[t, k])
    assert occ.dtype == f and stay.dtype == f
    return dict(occ=occ, stay=stay, adv=adv, logp=logp)


def occupancy64(p, init, y, band=0, path=None):
    """p: (T, S, N) float32 posteriors, init: (n_init,), y: the labels -> the definition in float64"""
    return _occupancy(p, init, y, band, path, np.float64)


def occupancy32(p, init, y, band=0, path=None):
    """the stated arithmetic in float32"""
    return _occupancy(p, init, y, band, path, np.float32)


def enumerate_occupancy(p, init, y):
    """every alignment of a tiny case -> (occ (T, S, N), adv (T, L), P): the summed weight of the alignments through each
    edge, divided by their total"""
    p = np.asarray(p, np.float32)
    T, S, N = p.shape
    y = [int(v) for v in y]
    L = len(y)
    sig = R.trajectory(init, y, S, N)
    occ, adv, total = np.zeros((T, S, N)), np.zeros((T, L)), 0.0
    for w, rows in R.enumerate_alignments(p, init, y):
        total += w
        k = 0
        for t in range(T):
            if k < L and rows[k] == t:
                if 0 <= sig[k] < S:
                    occ[t, sig[k], y[k]] += w
                adv[t, k] += w
                k += 1
            elif 0 <= sig[k] < S:
                occ[t, sig[k], 0] += w
    if not total > 0:
        return None, None, total
    return occ / total, adv / total, total
