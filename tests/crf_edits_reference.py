"""TEST INFRASTRUCTURE: what fcd_crf_edits_* computes (include/fcd.h), restated twice in float64 -- the specification the
kernels (csrc/crf_posterior.hip) are held to.

rescored():  exact mode straight from the definition: every variant labelling (y without label k; y with c before y_g) is
             scored on its own by tests/crf_lattice_reference.crf_score, its trajectory computed from scratch.
chain():     the chain definition of include/fcd.h on dense arrays, any band: alpha on the forward window (y's window, the
             cone one state wider below), the deletion chains W on the deletion window (the cone one state wider above), the
             insertion chains U on y's own window.  The variants' model states come from the trajectory RULE, a step at a
             time from sigma_k -- no closed form here.  Rows are rescaled by exact powers of two; every accumulator carries
             an integer exponent of its own.
enumerated(): the sum over every alignment of every variant labelling (crf_lattice_reference.enumerate_alignments): what
             both are pinned to on tiny cases.

All return (deletion (L,), insertion (L + 1, N - 1), logp): float64 natural logarithms of the variants' probabilities (NOT
yet the ratio against logp), -inf for probability 0, NaN where a NaN enters; every entry NaN where logp is not finite."""
import math

import numpy as np

import crf_lattice_reference as R

LN2 = math.log(2.0)


def variants(y, N):
    """-> ([y without k], [[y with c before y_g for c in 1 .. N-1] for g in 0 .. L])"""
    y = [int(v) for v in y]
    return [y[:k] + y[k + 1:] for k in range(len(y))], [[y[:g] + [c] + y[g:] for c in range(1, N)] for g in range(len(y) + 1)]


def _nan(L, N):
    return np.full(L, math.nan), np.full((L + 1, N - 1), math.nan)


def rescored(p, init, y):
    p = np.asarray(p)
    N = p.shape[2]
    y = [int(v) for v in y]
    logp = R.crf_score(p, init, y)
    dele, ins = _nan(len(y), N)
    if not math.isfinite(logp):
        return dele, ins, logp
    dv, iv = variants(y, N)
    for k, v in enumerate(dv):
        dele[k] = R.crf_score(p, init, v)
    for g, row in enumerate(iv):
        for c, v in enumerate(row):
            ins[g, c] = R.crf_score(p, init, v)
    return dele, ins, logp


def enumerated(p, init, y):
    p = np.asarray(p)
    N = p.shape[2]
    T = p.shape[0]

    def total(v):
        if len(v) > T:
            return -math.inf
        w = sum(a for a, _ in R.enumerate_alignments(p, init, v))
        return math.log(w) if w > 0 else (-math.inf if w == 0 else math.nan)

    dv, iv = variants(y, N)
    return (np.array([total(v) for v in dv], np.float64).reshape(len(dv)),
            np.array([[total(v) for v in row] for row in iv], np.float64), total([int(v) for v in y]))


def chain_depth(S, nb):
    if S == 1:
        return 1
    m, v = 0, 1
    while v < S:
        v *= nb
        m += 1
    assert v == S and nb >= 2, "S must be a power of N - 1"
    return m


def windows(t, T, L, band, path):
    """-> (y's window, the forward window, the deletion walk's window) of row t; t = -1: state 0 (and state 1 above it)"""
    lo, hi = 0, L
    if band:
        k = 0 if t < 0 else np.searchsorted(np.asarray(path, np.int64), t, side="right")
        lo, hi = max(0, int(k) - band), min(L, int(k) + band)
    cone = L - (T - 1 - t)
    return (max(lo, cone), min(hi, t + 1)), (max(lo, cone - 1), min(hi, t + 1)), (max(lo, cone), min(hi, t + 2))


def _mask(n, w):
    m = np.zeros(n, bool)
    if w[0] <= w[1]:
        m[max(w[0], 0):w[1] + 1] = True
    return m


def _rescale(arrs):
    """the arrays scaled by one exact power of two so that the largest positive finite value lies in [0.5, 1) -> exponent"""
    top = 0.0
    for a in arrs:
        good = a[np.isfinite(a) & (a > 0)]
        if good.size:
            top = max(top, float(good.max()))
    if top == 0.0:
        return 0
    e = int(np.frexp(top)[1])
    for a in arrs:
        a[...] = np.ldexp(a, -e)
    return e


class _Acc:
    """non-negative accumulators, each with an integer exponent of its own"""

    def __init__(self, shape):
        self.v = np.zeros(shape)
        self.e = np.full(shape, -(1 << 40), np.int64)

    def add(self, term, e):
        tm, te = np.frexp(term)
        te = te.astype(np.int64) + e
        pos = np.isfinite(term) & (term > 0)
        ne = np.where(pos, np.maximum(self.e, te), self.e)
        self.v = np.ldexp(self.v, np.clip(self.e - ne, -5000, 0).astype(np.int32)) + \
            np.where(term == 0, 0.0, np.ldexp(tm, np.clip(te - ne, -5000, 5000).astype(np.int32)))
        self.e = ne

    def ln(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.v == 0, -math.inf, np.log(self.v) + self.e * LN2)


def chain(p, init, y, band=0, path=None):
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.ndim == 3
    T, S, N = p.shape
    nb = N - 1
    y = [int(v) for v in y]
    L = len(y)
    logp = R.crf_score(p, init, y, band, path)
    dele, ins = _nan(L, N)
    if not math.isfinite(logp):
        return dele, ins, logp
    m = chain_depth(S, nb)
    sig = R.trajectory(init, y, S, N)
    pd = p.astype(np.float64)
    p0, py = R._rows(p, sig, y)
    p0 = np.concatenate([p0.astype(np.float64), np.zeros((T, 1))], 1)  # (state L + 1: nothing)
    py = np.concatenate([py.astype(np.float64), np.zeros((T, 1))], 1)
    ycol = np.array(y + [0, 0], np.int64)
    intab = np.array([0 <= s < S for s in sig] + [False])
    sigc = np.where(intab, np.array(sig + [0]), 0)
    # the variants' model states, by the rule: insertion slot s = g + j, deletion slot s = k + 2 + j
    svI = np.full((L + 2, m, nb), -1, np.int64)
    for g in range(L + 1):
        for c in range(nb):
            s = (sig[g] * nb) % S + c
            for j in range(m):
                if g + j > L:
                    break
                svI[g + j, j, c] = s if 0 <= s < S else -1
                if g + j < L:
                    s = (s * nb) % S + (y[g + j] - 1)
    svD = np.full((L + 2, max(m - 1, 1)), -1, np.int64)
    for k in range(L - 1):
        s = (sig[k] * nb) % S + (y[k + 1] - 1)
        for j in range(m - 1):
            if k + 2 + j > L:
                break
            svD[k + 2 + j, j] = s if 0 <= s < S else -1
            if k + 2 + j < L:
                s = (s * nb) % S + (y[k + 2 + j] - 1)
    okI, okD = svI >= 0, svD >= 0
    PI0 = np.where(okI, pd[:, svI.clip(0), 0], 0.0)                                  # (T, L+2, m, nb)
    PIy = np.where(okI & (ycol[:, None, None] > 0), pd[:, svI.clip(0), ycol[:, None, None]], 0.0)
    PD0 = np.where(okD, pd[:, svD.clip(0), 0], 0.0)                                  # (T, L+2, m-1)
    PDy = np.where(okD & (ycol[:, None] > 0), pd[:, svD.clip(0), ycol[:, None]], 0.0)
    Pe = np.where(intab[:, None], pd[:, sigc, 1:], 0.0)                              # (T, L+2, nb): state g emits c
    Pd = np.where((intab & (np.arange(L + 2) < L - 1))[None, :], pd[:, sigc, np.roll(ycol, -1)], 0.0)  # state k emits y_{k+1}
    n = L + 2

    # ---- forward, on the forward window ----
    A, EA = np.zeros((T, n)), np.zeros(T, np.int64)
    a = np.zeros(n)
    a[0] = 1.0
    pm, e_tot = _mask(n, (0, 0)), 0
    for t in range(T):
        wm = _mask(n, windows(t, T, L, band, path)[1])
        src = np.where(pm, a, 0.0)
        nw = src * p0[t]
        nw[1:] = nw[1:] + (src * py[t])[:-1]
        nw = np.where(wm, nw, 0.0)
        e_tot += _rescale([nw])
        A[t], EA[t] = nw, e_tot
        a, pm = nw, wm

    def masks(u, which):
        wu = windows(u, T, L, band, path)[which]
        wp = windows(u - 1, T, L, band, path)[which]
        if u == 0 and which == 0:
            wp = (0, 0)
        mu, mp = _mask(n, wu), _mask(n, wp)
        own = mp & mu
        nxt = mp.copy()
        nxt[:-1] &= mu[1:]
        nxt[-1] = False
        return own, nxt, mp

    def alpha_before(u):
        if u == 0:
            a0 = np.zeros(n)
            a0[0] = 1.0
            return a0, 0
        return np.where(_mask(n, windows(u - 1, T, L, band, path)[1]), A[u - 1], 0.0), int(EA[u - 1])

    def up(x):  # the next state's value
        return np.concatenate([x[1:], np.zeros((1,) + x.shape[1:])], 0)

    last = np.zeros(n)
    last[L] = 1.0
    # ---- insertions ----
    chainI = np.zeros((n, m, nb), bool)
    for s in range(L + 1):
        chainI[s, :min(m, s + 1)] = True
    b, U = last.copy(), np.where(chainI, last[:, None, None], 0.0)
    accI, eb = _Acc((n, nb)), 0
    for u in range(T - 1, -1, -1):
        own, nxt, live = masks(u, 0)
        av, ea = alpha_before(u)
        carry = live & own                                                    # gap g holds a value at row u and at row u - 1
        accI.add(np.where(carry[:, None], av[:, None] * Pe[u] * U[:, 0, :], 0.0), ea + eb)
        upU = np.concatenate([up(U)[:, 1:, :], np.broadcast_to(up(b)[:, None, None], (n, 1, nb))], 1)
        nU = np.where(own[:, None, None], PI0[u] * U, 0.0) + np.where(nxt[:, None, None], PIy[u] * upU, 0.0)
        nU = np.where(chainI, nU, 0.0)
        nbeta = np.where(own, p0[u] * b, 0.0) + np.where(nxt, py[u] * up(b), 0.0)
        eb += _rescale([nbeta, nU])
        b, U = nbeta, nU
    ins = accI.ln()[:L + 1]
    # ---- deletions ----
    J = max(m - 1, 1)
    chainD = np.zeros((n, J), bool)
    for s in range(2, L + 1):
        chainD[s, :min(m - 1, s - 1)] = True
    b, W = last.copy(), np.where(chainD, last[:, None], 0.0)
    accD, eb = _Acc(n), 0
    for u in range(T - 1, -1, -1):
        own, nxt, live = masks(u, 2)
        av, ea = alpha_before(u)
        mu = _mask(n, windows(u, T, L, band, path)[2])
        X = W[:, 0] if m > 1 else b
        x2 = np.where(np.concatenate([mu[2:], [False, False]]), np.concatenate([X[2:], [0.0, 0.0]]), 0.0)  # X_u[k + 2]
        carry = np.concatenate([live[1:], [False]])                           # the carrying state k + 1, at row u - 1
        accD.add(np.where(carry & (np.arange(n) < L - 1), av * Pd[u] * x2, 0.0), ea + eb)
        upW = np.concatenate([up(W)[:, 1:], up(b)[:, None]], 1) if m > 1 else W
        nW = np.where(own[:, None], PD0[u] * W, 0.0) + np.where(nxt[:, None], PDy[u] * upW, 0.0)
        nW = np.where(chainD, nW, 0.0)
        nbeta = np.where(own, p0[u] * b, 0.0) + np.where(nxt, py[u] * up(b), 0.0)
        eb += _rescale([nbeta, nW])
        b, W = nbeta, nW
    dele = accD.ln()[:L].copy()
    if L >= 1:  # the last label: the shortened labelling's final state, off the last forward row
        v = A[T - 1, L - 1] if _mask(n, windows(T - 1, T, L, band, path)[1])[L - 1] else 0.0
        dele[L - 1] = (math.log(v) + int(EA[T - 1]) * LN2) if v > 0 else (-math.inf if v == 0 else math.nan)
    return dele, ins, logp
