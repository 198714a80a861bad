"""TEST INFRASTRUCTURE: what fcd_crf_transition_probs_* computes (include/fcd.h), restated in numpy -- the specification
the kernel (csrc/crf_transitions.hip, crf_transitions_walk) is held to.

  transitions64(x)   the formulas as the header states them, in float64, no renormalisation: the reference of every check
  transitions32(x)   the stated ARITHMETIC in float32: beta renormalised by its row maximum at every step, per state
                     m = max y, e = exp(y - m), the sum in the order a = 0 .. N - 1, p = e / sum, beta = m + ln sum, logZ the
                     float64 sum of the row maxima + ln sum exp beta~_0.  Its distance to transitions64 is err32, the unit of
                     the kernel's allowance (tests/crf_transitions_cases.py)
  dest_to_source / source_to_dest   the two score layouts
  enumerate_paths(x) every start state and symbol sequence of a tiny case with its score sum

x: (T, S, N) scores in log space, source-indexed.  -inf is a forbidden transition.  Both restatements return
dict(probs (T, S, N), init (S,), logz, ok); ok False (and logz NaN) for a read the definition fails: a row of beta with no
live state, or a NaN / +inf score."""
import itertools

import numpy as np


def destinations(S, N):
    """d[s][a]: the state symbol a leaves state s in -- s for a = 0, (s nb) mod S + a - 1 otherwise"""
    nb = N - 1
    s = np.arange(S)
    d = np.empty((S, N), np.int64)
    d[:, 0] = s
    for j in range(nb):
        d[:, j + 1] = (s * nb) % S + j
    return d


def _dest_index(S, N):
    """(rows, cols): x[..., s, a] = xd[..., rows[s, a], cols[s, a]]"""
    nb = N - 1
    d = destinations(S, N)
    cols = np.zeros((S, N), np.int64)
    cols[:, 1:] = (1 + (np.arange(S) * nb) // S)[:, None]
    return d, cols


def dest_to_source(xd):
    """scores indexed by the state being entered -> by the state being left (the last two axes are (S, N))"""
    S, N = xd.shape[-2:]
    rows, cols = _dest_index(S, N)
    return xd[..., rows, cols]


def source_to_dest(x):
    S, N = x.shape[-2:]
    rows, cols = _dest_index(S, N)
    xd = np.empty_like(x)
    xd[..., rows, cols] = x
    return xd


def _failed(S, N, T, dtype):
    return dict(probs=np.full((T, S, N), np.nan, dtype), init=np.full(S, np.nan, dtype), logz=float("nan"), ok=False)


def transitions64(x):
    x = np.asarray(x, np.float64)
    T, S, N = x.shape
    if np.isnan(x).any() or (x == np.inf).any():
        return _failed(S, N, T, np.float64)
    d = destinations(S, N)
    beta = np.zeros(S)
    probs = np.zeros((T, S, N))
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T - 1, -1, -1):
            y = x[t] + beta[d]
            m = y.max(axis=1)
            live = m > -np.inf
            if not live.any():
                return _failed(S, N, T, np.float64)
            e = np.where(live[:, None], np.exp(y - np.where(live, m, 0.0)[:, None]), 0.0)
            z = e.sum(axis=1)
            probs[t] = np.where(live[:, None], e / np.where(live, z, 1.0)[:, None], 0.0)
            beta = np.where(live, m + np.log(np.where(live, z, 1.0)), -np.inf)
        c = beta.max()
        z = np.exp(beta - c).sum()
        logz = c + np.log(z)
        init = np.exp(beta - logz)
    return dict(probs=probs, init=init, logz=float(logz), ok=True)


def transitions32(x, renormalise=True):
    """the stated arithmetic in float32 (renormalise=False: without the per-row maximum, to show what it is for)"""
    f = np.float32
    x = np.asarray(x, f)
    T, S, N = x.shape
    bad = bool(np.isnan(x).any() or (x == np.inf).any())
    d = destinations(S, N)
    beta = np.zeros(S, f)
    probs = np.zeros((T, S, N), f)
    csum = 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            y = (x[t] + beta[d]).astype(f)
            m = y.max(axis=1)
            live = m > -np.inf
            e = np.where(live[:, None], np.exp((y - np.where(live, m, f(0))[:, None]).astype(f)), f(0)).astype(f)
            z = np.zeros(S, f)
            for a in range(N):  # in the order a = 0 .. N - 1
                z = (z + e[:, a]).astype(f)
            zz = np.where(live, z, f(1))
            probs[t] = np.where(live[:, None], (e / zz[:, None]).astype(f), f(0))
            beta = np.where(live, (m + np.log(zz).astype(f)).astype(f), f(-np.inf)).astype(f)
            c = beta.max() if renormalise else f(0)
            if not (c > -np.inf):
                bad = True
                break
            csum += float(c)
            beta = (beta - c).astype(f)
        if bad:
            return _failed(S, N, T, f)
        e0 = np.exp(beta).astype(f)
        z = e0.sum(dtype=f)
        init = (e0 / z).astype(f)
        logz = csum + float(np.log(np.float64(z)))
    return dict(probs=probs, init=init, logz=logz, ok=True)


def enumerate_paths(x):
    """every (start state, symbol sequence) of a tiny case -> (s0, symbols, states, score sum), float64"""
    x = np.asarray(x, np.float64)
    T, S, N = x.shape
    d = destinations(S, N)
    out = []
    for s0 in range(S):
        for sym in itertools.product(range(N), repeat=T):
            s, total, states = s0, 0.0, []
            for t, a in enumerate(sym):
                states.append(s)
                total += x[t, s, a]
                s = int(d[s, a])
            out.append((s0, sym, states, total))
    return out


def random_scores(rng, T, S, N, sd=2.0, n_neg_inf=0, dead=None):
    """sd N(0, 1) scores; n_neg_inf entries forbidden; dead = (t, s): every candidate of that state at that row forbidden"""
    x = (sd * rng.standard_normal((T, S, N))).astype(np.float32)
    if n_neg_inf and x.size:
        idx = rng.choice(x.size, size=min(n_neg_inf, x.size), replace=False)
        x.reshape(-1)[idx] = -np.inf
    if dead is not None and T:
        x[dead[0], dead[1], :] = -np.inf
    return x
