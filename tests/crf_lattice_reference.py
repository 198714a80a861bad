"""TEST INFRASTRUCTURE: what fcd_crf_score_* / fcd_crf_align_* compute (include/fcd.h), restated in numpy straight from the
definition -- the specification the kernels (csrc/crf_lattice.hip) are held to -- and a brute-force enumerator of every
alignment of a tiny case.

The labelling y of L labels walks the model states sigma_0 = first argmax of the init row, sigma_{k+1} = (sigma_k nb) mod S
+ (y_k - 1); P(t, k, j) = p[t][sigma_k][j], 0 where sigma_k lies outside 0 .. S-1.  States k = 0 .. L:
    alpha_{-1}[0] = 1,   alpha_t[k] = alpha_{t-1}[k] P(t,k,0) + alpha_{t-1}[k-1] P(t,k-1,y_{k-1})
Score: the sum, in float64 (rows rescaled by powers of two, exact).  Align: max in place of +, a value being an f32 mantissa
in [0.5, 1) (np.float32, so that a product rounds as the kernel's does) with a Python-int exponent -- "f32 with an unbounded
exponent"; each of the two candidates is ONE f32 product; the stay candidate is kept unless the advance candidate is
strictly greater.  Window of row t (band = W >= 1, k(t) = #{k : path[k] <= t}): max(0, k(t)-W) .. min(L, k(t)+W), cut to
k <= t + 1 (reachable) and k >= L - (T-1-t) (can still reach the end); everything else counts as 0."""
import bisect
import itertools
import math

import numpy as np

ZERO_E = -(1 << 40)  # exponent of a zero cell: below every real one


def trajectory(init, y, S, N):
    """sigma_0 .. sigma_L (plain ints; values outside 0 .. S-1 are kept as they are)"""
    init = [-math.inf if v != v else float(v) for v in np.asarray(init, np.float32)]  # (a NaN counts as -inf)
    best = 0
    for i, v in enumerate(init):  # the first maximum
        if v > init[best]:
            best = i
    nb = N - 1
    sig = [best]
    for v in y:
        sig.append((sig[-1] * nb) % S + (int(v) - 1))
    return sig


def window(t, T, L, band, path):
    lo, hi = 0, L
    if band:
        k = bisect.bisect_right(path, t)
        lo, hi = max(0, k - band), min(L, k + band)
    return max(lo, L - (T - 1 - t)), min(hi, t + 1)


def _early(p, y, N):
    """the rows without a value that both walks share -> a logp, or None"""
    T, L = p.shape[0], len(y)
    if any(not 1 <= v < N for v in y):
        return math.nan
    if T == 0:
        return 0.0 if L == 0 else -math.inf
    if L > T:
        return -math.inf
    return None


def _rows(p, sig, y):
    """P(t, k, 0) and P(t, k, y_k) as (T, L + 1) float32 arrays (column L of the second is 0)"""
    T, S, N = p.shape
    L = len(y)
    p0 = np.zeros((T, L + 1), np.float32)
    py = np.zeros((T, L + 1), np.float32)
    for k in range(L + 1):
        if 0 <= sig[k] < S:
            p0[:, k] = p[:, sig[k], 0]
            if k < L:
                py[:, k] = p[:, sig[k], y[k]]
    return p0, py


def crf_score(p, init, y, band=0, path=None):
    """p: (T, S, N) float32, init: (n_init,) -> ln alpha_{T-1}[L] in float64"""
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.ndim == 3
    T, S, N = p.shape
    y = [int(v) for v in y]
    L = len(y)
    early = _early(p, y, N)
    if early is not None:
        return early
    if band:
        path = [int(v) for v in path]
        assert len(path) == L
    p0, py = _rows(p, trajectory(init, y, S, N), y)
    p0, py = p0.astype(np.float64), py.astype(np.float64)
    a = np.zeros(L + 1)
    a[0] = 1.0
    plo, phi, e_tot = 0, 0, 0
    for t in range(T):
        lo, hi = window(t, T, L, band, path)
        n = np.zeros(L + 1)
        for k in range(lo, hi + 1):
            v = 0.0
            if plo <= k <= phi:
                v = a[k] * p0[t, k]
            if k >= 1 and plo <= k - 1 <= phi:
                v = v + a[k - 1] * py[t, k - 1]
            n[k] = v
        good = n[np.isfinite(n) & (n > 0)]
        if good.size:
            e = int(np.frexp(good.max())[1])
            n = np.ldexp(n, -e)
            e_tot += e
        a, plo, phi = n, lo, hi
    m = a[L] if plo <= L <= phi else 0.0
    if m != m:
        return math.nan
    return (math.log(m) if m > 0 else -math.inf) + e_tot * math.log(2.0)


def _gt(m1, e1, m0, e0):
    return e1 > e0 or (e1 == e0 and m1 > m0)


def _mul(am, ae, v):
    """(mantissa, exponent) of the f32-with-unbounded-exponent product of a cell and a finite posterior v >= 0"""
    if not am > 0 or not v > 0:
        return np.float32(0), ZERO_E
    pm, pe = np.frexp(np.float32(v))
    prod = np.float32(am) * np.float32(pm)  # f32 x f32: one rounding
    assert prod.dtype == np.float32
    fm, fe = np.frexp(prod)
    return np.float32(fm), int(ae) + int(pe) + int(fe)


def crf_align(p, init, y, band=0, path=None, drop=None):
    """-> dict(logp, start, count, qual (np.float32)); start / count / qual are None where there is no alignment"""
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.ndim == 3
    T, S, N = p.shape
    y = [int(v) for v in y]
    L = len(y)
    none = dict(start=None, count=None, qual=None)
    early = _early(p, y, N)
    if early is not None:
        if early == 0.0:
            return dict(logp=0.0, start=[], count=[], qual=[])
        return dict(none, logp=early)
    if band:
        path = [int(v) for v in path]
        assert len(path) == L
    sig = trajectory(init, y, S, N)
    p0, py = _rows(p, sig, y)
    am = [np.float32(0)] * (L + 1)
    ae = [ZERO_E] * (L + 1)
    am[0], ae[0] = np.float32(0.5), 1  # "row -1": 1.0 on state 0
    bp = np.zeros((T, L + 1), np.uint8)
    plo, phi = 0, 0
    bad = False
    for t in range(T):
        lo, hi = window(t, T, L, band, path)
        nm = [np.float32(0)] * (L + 1)
        ne = [ZERO_E] * (L + 1)
        for k in range(lo, hi + 1):
            sm, se, vm, ve = np.float32(0), ZERO_E, np.float32(0), ZERO_E
            if plo <= k <= phi:
                v = p0[t, k]
                if not (np.isfinite(v) and v >= 0):
                    bad = True
                else:
                    sm, se = _mul(am[k], ae[k], v)
            if k >= 1 and plo <= k - 1 <= phi:
                v = py[t, k - 1]
                if not (np.isfinite(v) and v >= 0):
                    bad = True
                else:
                    vm, ve = _mul(am[k - 1], ae[k - 1], v)
            if _gt(vm, ve, sm, se):
                nm[k], ne[k], bp[t, k] = vm, ve, 1
            else:
                nm[k], ne[k] = sm, se
        if drop is not None:
            live = [k for k in range(lo, hi + 1) if nm[k] > 0]
            if live:
                top = max(live, key=lambda k: (ne[k], nm[k]))
                cut = int(round(math.log2(drop)))
                assert 2.0 ** cut == drop
                for k in live:
                    if _gt(nm[top], ne[top] + cut, nm[k], ne[k]):
                        nm[k], ne[k] = np.float32(0), ZERO_E
        am, ae, plo, phi = nm, ne, lo, hi
    if bad:
        return dict(none, logp=math.nan)
    if not (plo <= L <= phi) or not am[L] > 0:
        return dict(none, logp=-math.inf)
    logp = math.log(float(am[L])) + int(ae[L]) * math.log(2.0)
    start = [None] * L
    k = L
    for t in range(T - 1, -1, -1):
        if bp[t, k]:
            start[k - 1] = t
            k -= 1
    assert k == 0
    qual = [np.float32(py[start[k], k]) for k in range(L)]
    return dict(logp=logp, start=start, count=[1] * L, qual=qual)


def enumerate_alignments(p, init, y):
    """every alignment (the emission rows e_0 < ... < e_{L-1}) of labelling y over the T rows of p with its float64
    probability, in itertools.combinations order"""
    p = np.asarray(p, np.float32)
    T, S, N = p.shape
    y = [int(v) for v in y]
    L = len(y)
    p0, py = _rows(p, trajectory(init, y, S, N), y)
    p0, py = p0.astype(np.float64), py.astype(np.float64)
    out = []
    for rows in itertools.combinations(range(T), L):
        w, k = 1.0, 0
        for t in range(T):
            if k < L and rows[k] == t:
                w *= py[t, k]
                k += 1
            else:
                w *= p0[t, k]
        out.append((w, rows))
    return out
