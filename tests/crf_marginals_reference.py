"""TEST INFRASTRUCTURE: what fcd_crf_marginals_* computes (include/fcd.h), restated in numpy -- the specification the kernel
(csrc/crf_transitions.hip, crf_marginals_kernel) is held to.

  marginals64(x)     the alpha / beta definition as the header states it, in float64 log space: the reference of every check.
                     It never forms p or init.
  marginals32(x)     the stated ARITHMETIC in float32: (p, init) of crf_transitions_reference.transitions32, then
                     pi_0 = init, marg[t][s][a] = pi_t[s] p[t][s][a], pi_{t+1}[s'] = marg[t][s'][0] + sum_i marg[t][s_i][j+1]
                     taken left to right from the stay term on; emit a float32 sum over states.  Its distance to
                     marginals64 is err32, the unit of the kernel's allowance (tests/crf_marginals_cases.py)
  propagate32(p, init)   the forward half alone, on any (probs, init) pair: what the kernel does to crf_transition_probs'
                     own output, bit for bit (one rounding per product and per sum, no fused multiply-add)
  enumerate_marginals(x) the summed weight of the paths through every edge of a tiny case over Z, by enumeration

x: (T, S, N) scores in log space, source-indexed.  -inf is a forbidden transition.  The restatements return
dict(marg (T, S, N), emit (T, N), logz, ok); ok False (and logz NaN) for a read the definition fails: no path of positive
weight, or a NaN / +inf score."""
import numpy as np

import crf_transitions_reference as R


def _failed(S, N, T, dtype):
    return dict(marg=np.full((T, S, N), np.nan, dtype), emit=np.full((T, N), np.nan, dtype), logz=float("nan"), ok=False)


def _lse(y, axis):
    """ln sum exp along an axis; -inf where every term is -inf"""
    m = y.max(axis=axis, keepdims=True)
    m0 = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return (m0 + np.log(np.exp(y - m0).sum(axis=axis, keepdims=True))).squeeze(axis)


def marginals64(x):
    x = np.asarray(x, np.float64)
    T, S, N = x.shape
    if np.isnan(x).any() or (x == np.inf).any():
        return _failed(S, N, T, np.float64)
    d = R.destinations(S, N)
    with np.errstate(invalid="ignore", divide="ignore"):
        beta = np.zeros((T + 1, S))
        for t in range(T - 1, -1, -1):
            beta[t] = _lse(x[t] + beta[t + 1][d], 1)
        logz = float(_lse(beta[0], 0))
        if not logz > -np.inf:
            return _failed(S, N, T, np.float64)
        alpha = np.zeros((T + 1, S))
        for t in range(T):
            v = alpha[t][:, None] + x[t]  # (S, N): the terms of alpha_{t+1}[d(s, a)]
            mx = np.full(S, -np.inf)
            np.maximum.at(mx, d, v)
            m0 = np.where(np.isfinite(mx), mx, 0.0)
            acc = np.zeros(S)
            np.add.at(acc, d, np.exp(v - m0[d]))
            alpha[t + 1] = np.where(acc > 0, m0 + np.log(np.where(acc > 0, acc, 1.0)), -np.inf)
        marg = np.zeros((T, S, N))
        for t in range(T):
            marg[t] = np.exp(alpha[t][:, None] + x[t] + beta[t + 1][d] - logz)
        marg[np.isnan(marg)] = 0.0  # (-inf - -inf cannot arise: logz is finite; kept for the forbidden entries' sake)
    return dict(marg=marg, emit=marg.sum(axis=1), logz=logz, ok=True, alpha=alpha, beta=beta)


def logz64(x):
    """ln of the sum over every start state and symbol sequence of exp(score), float64"""
    x = np.asarray(x, np.float64)
    d = R.destinations(x.shape[1], x.shape[2])
    beta = np.zeros(x.shape[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(x.shape[0] - 1, -1, -1):
            beta = _lse(x[t] + beta[d], 1)
        return float(_lse(beta, 0))


def propagate32(probs, init):
    """(T, S, N) float32 transition posteriors and the (S,) float32 init row -> (marg, emit) float32: the device's forward
    pass, product by product and sum by sum"""
    f = np.float32
    p = np.asarray(probs, f)
    T, S, N = p.shape
    nb = N - 1
    q = S // nb
    s2 = np.arange(S)
    hi, j = s2 // nb, s2 % nb
    pi = np.asarray(init, f).copy()
    marg = np.zeros((T, S, N), f)
    for t in range(T):
        m = (pi[:, None] * p[t]).astype(f)
        marg[t] = m
        nx = m[:, 0].copy()
        for i in range(nb):
            nx = (nx + m[hi + i * q, j + 1]).astype(f)
        pi = nx
    return marg, marg.sum(axis=1, dtype=f)


def marginals32(x, transitions=None):
    """the stated arithmetic in float32; `transitions`: R.transitions32(x) where the caller has it already"""
    x = np.asarray(x, np.float32)
    T, S, N = x.shape
    tr = R.transitions32(x) if transitions is None else transitions
    if not tr["ok"]:
        return _failed(S, N, T, np.float32)
    marg, emit = propagate32(tr["probs"], tr["init"])
    return dict(marg=marg, emit=emit, logz=tr["logz"], ok=True)


def enumerate_marginals(x):
    """every start state and symbol sequence of a tiny case -> (marg (T, S, N), Z's logarithm): the summed weight of the paths
    through each edge, divided by Z"""
    x = np.asarray(x, np.float64)
    T, S, N = x.shape
    paths = R.enumerate_paths(x)
    top = max(p[3] for p in paths)
    w = np.zeros((T, S, N))
    z = 0.0
    for s0, sym, states, score in paths:
        e = np.exp(score - top)
        z += e
        for t, a in enumerate(sym):
            w[t, states[t], a] += e
    return w / z, top + np.log(z)
