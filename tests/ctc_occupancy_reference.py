"""TEST INFRASTRUCTURE: the label occupancies fcd_ctc_occupancy_* computes (include/fcd.h), restated in float64 numpy
straight from their definition, in the log domain (no row scales, nothing dropped: it shares no code with the kernel's
scaling) -- the specification the walk (csrc/ctc_posterior.hip, ctc_occ_walk) is held to -- and a brute-force enumerator
over every alignment of a tiny case.

Extended sequence z of 2L + 1 states (z[2k] = blank, z[2k+1] = y[k]); "row -1" holds 1 on state 0, "row T" 1 on state 2L.
    enter(s)   from s (a blank, or collapse), s - 1, and s - 2 where s is a label state, s >= 3 and (no collapse or z[s] != z[s-2])
    alpha_t[s] = (sum over enter(s) of alpha_{t-1}) * p[t][z[s]]
    beta_t[s]  = sum over the s' with s in enter(s') of beta_{t+1}[s'] * p[t+1][z[s']]           (row T: the 1 on state 2L)
    P          = alpha_{T-1}[2L] + alpha_{T-1}[2L-1]
    gamma_t[s] = alpha_t[s] * beta_t[s] / P,    occ[t][c] = sum over the s with z[s] = c of gamma_t[s]
band = W >= 1: with k(t) = #{k : path[k] <= t}, states outside max(0, 2(k(t)-W)-2) .. min(2L, 2(k(t)+W)) count as 0 at row t,
in alpha and in beta alike (tests/ctc_score_reference.py's window)."""
import bisect
import itertools
import math

import numpy as np

import ctc_score_reference as R

NEG = -math.inf


def _lse(*terms):
    out = terms[0]
    for t in terms[1:]:
        out = np.logaddexp(out, t)
    return out


def _from_below(a, n):
    """out[s] = a[s - n], -inf where there is no such state"""
    return np.concatenate((np.full(n, NEG), a))[:a.size]


def _from_above(a, n):
    """out[s] = a[s + n]"""
    return np.concatenate((a, np.full(n, NEG)))[n:]


def occupancy64(p, y, collapse_repeats=True, band=0, path=None):
    """p: (T, N) posteriors (used as float64), y: labels 1 .. N-1 -> dict(logp, occ (T, N) float64 or None where P is not
    positive and finite or T = 0, gamma (T, 2L+1))"""
    p = np.asarray(p, np.float64)
    T, N = p.shape
    y = [int(v) for v in y]
    L = len(y)
    if any(not 1 <= v < N for v in y):
        return dict(logp=math.nan, occ=None, gamma=None)
    if T == 0:
        return dict(logp=0.0 if L == 0 else NEG, occ=None, gamma=None)
    S = 2 * L + 1
    z = np.zeros(S, np.int64)
    z[1::2] = y
    odd = (np.arange(S) & 1).astype(bool)
    skip = np.zeros(S, bool)  # skip[s]: s - 2 enters s
    for s in range(3, S, 2):
        skip[s] = (z[s] != z[s - 2]) if collapse_repeats else True
    stay = np.ones(S, bool) if collapse_repeats else ~odd
    live = np.ones((T, S), bool)
    if band:
        path = [int(v) for v in path]
        assert len(path) == L
        for t in range(T):
            k = bisect.bisect_right(path, t)
            lo, hi = max(0, 2 * (k - band) - 2), min(2 * L, 2 * (k + band))
            live[t] = False
            live[t, lo:hi + 1] = True
    with np.errstate(all="ignore"):
        lpz = np.log(p[:, z])  # (T, S); log 0 = -inf, a NaN stays one
        la = np.full((T, S), NEG)
        prev = np.full(S, NEG)
        prev[0] = 0.0
        for t in range(T):
            s1 = _from_below(prev, 1)
            s2 = np.where(skip, _from_below(prev, 2), NEG)
            tot = _lse(np.where(stay, prev, NEG), s1, s2)
            la[t] = np.where(live[t], tot + lpz[t], NEG)
            prev = la[t]
        logp = float(_lse(la[T - 1, 2 * L], la[T - 1, 2 * L - 1] if L > 0 else NEG))
        lbeta = np.full((T, S), NEG)
        nb = np.full(S, NEG)  # ln b_{t+1}
        nb[2 * L] = 0.0
        for t in range(T - 1, -1, -1):
            u1 = _from_above(nb, 1)
            u2 = _from_above(np.where(skip, nb, NEG), 2)  # s -> s + 2 where skip[s + 2]
            lbeta[t] = np.where(live[t], _lse(np.where(stay, nb, NEG), u1, u2), NEG)
            nb = np.where(live[t], lbeta[t] + lpz[t], NEG)
        if not math.isfinite(logp):
            return dict(logp=logp if logp == NEG else math.nan, occ=None, gamma=None)
        gamma = np.exp(la + lbeta - logp)
        gamma[~live] = 0.0
        occ = np.zeros((T, N))
        for s in range(S):
            occ[:, z[s]] += gamma[:, s]
    return dict(logp=logp, occ=occ, gamma=gamma)


def brute_force(p, y, collapse_repeats=True):
    """-> (P, occ (T, N)) summed over every alignment of y, one by one"""
    p = np.asarray(p, np.float64)
    T, N = p.shape
    want = tuple(int(v) for v in y)
    P = 0.0
    occ = np.zeros((T, N))
    for pi in itertools.product(range(N), repeat=T):
        if R.collapse_alignment(pi, collapse_repeats) != want:
            continue
        w = 1.0
        for t, c in enumerate(pi):
            w *= p[t, c]
        P += w
        for t, c in enumerate(pi):
            occ[t, c] += w
    return P, (occ / P if P > 0 else None)
