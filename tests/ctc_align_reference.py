"""TEST INFRASTRUCTURE: the CTC forced alignment fcd_ctc_align_* computes (include/fcd.h), restated in numpy straight from
its definition -- the specification the kernels (csrc/ctc_align.hip) are held to EXACTLY -- and a brute-force enumerator of
every alignment of a tiny case.

A value is an f32 mantissa in [0.5, 1) (np.float32, so that a product rounds as the kernel's does) with a Python-int
exponent: "f32 with an unbounded exponent".  A cell is max(candidates) * p, one f32 rounding of the mantissa product;
candidates in the order stay, s-1, s-2, a later one only if strictly greater; at the end state 2L unless 2L-1 is strictly
greater.  Window of row t (band = W >= 1, k(t) = #{k : path[k] <= t}): max(0, 2(k-W)-2) .. min(2L, 2(k+W)), cut to
s <= 2t+1 (reachable) and s >= 2L - 2(T-1-t) - 2 (can still reach the end); everything else counts as 0."""
import bisect
import math

import numpy as np

ZERO_E = -(1 << 40)  # exponent of a zero cell: below every real one


def _gt(m1, e1, m0, e0):
    return (e1 > e0) | ((e1 == e0) & (m1 > m0))


def ctc_align(p, y, collapse_repeats=True, band=0, path=None, drop=None):
    """p: (T, N) float32 posteriors, y: labels 1 .. N-1 -> dict(logp, start, count, qual (np.float32), states) --
    start / count / qual / states are None where there is no alignment (logp NaN or -inf)."""
    p = np.asarray(p)
    assert p.dtype == np.float32
    T, N = p.shape
    y = [int(v) for v in y]
    L = len(y)
    none = dict(start=None, count=None, qual=None, states=None)
    if any(not 1 <= v < N for v in y):
        return dict(none, logp=math.nan)
    if T == 0:
        return dict(none, logp=-math.inf) if L else dict(logp=0.0, start=[], count=[], qual=[], states=[])
    if L > T:
        return dict(none, logp=-math.inf)
    if not (np.isfinite(p).all() and (p >= 0).all()):
        return dict(none, logp=math.nan)
    S = 2 * L + 1
    z = np.zeros(S, np.int64)
    z[1::2] = y
    odd = (np.arange(S) & 1).astype(bool)
    skip = np.zeros(S, bool)
    for s in range(3, S, 2):
        skip[s] = (z[s] != z[s - 2]) if collapse_repeats else True
    if band:
        path = [int(v) for v in path]
        assert len(path) == L
    pm, pe = np.frexp(p)  # exact
    pe = pe.astype(np.int64)
    # cell s lives at index s + 2: two zeros in front stand for the states below 0
    am = np.zeros(S + 2, np.float32)
    ae = np.full(S + 2, ZERO_E, np.int64)
    am[2], ae[2] = np.float32(0.5), 1  # "row -1": 1.0 on state 0
    bp = np.zeros((T, S), np.uint8)
    for t in range(T):
        lo, hi = 0, 2 * L
        if band:
            k = bisect.bisect_right(path, t)
            lo, hi = max(0, 2 * (k - band) - 2), min(2 * L, 2 * (k + band))
        hi = min(hi, 2 * t + 1)
        lo = max(lo, 2 * L - 2 * (T - 1 - t) - 2)
        nm = np.zeros(S + 2, np.float32)
        ne = np.full(S + 2, ZERO_E, np.int64)
        if hi >= lo:
            sl = slice(lo, hi + 1)
            m0, e0 = am[lo + 2:hi + 3], ae[lo + 2:hi + 3]
            m1, e1 = am[lo + 1:hi + 2], ae[lo + 1:hi + 2]
            m2, e2 = am[lo:hi + 1], ae[lo:hi + 1]
            od, sk = odd[sl], skip[sl]
            no_stay = od & (not collapse_repeats)
            bm, be = np.where(no_stay, m1, m0), np.where(no_stay, e1, e0)
            arg = np.where(no_stay, 1, 0).astype(np.uint8)
            up = ~no_stay & _gt(m1, e1, bm, be)
            bm, be, arg = np.where(up, m1, bm), np.where(up, e1, be), np.where(up, 1, arg)
            up = sk & _gt(m2, e2, bm, be)
            bm, be, arg = np.where(up, m2, bm), np.where(up, e2, be), np.where(up, 2, arg)
            prod = bm.astype(np.float32) * pm[t][z[sl]]  # f32 x f32: one rounding
            assert prod.dtype == np.float32
            fm, fe = np.frexp(prod)
            live = prod > 0
            cm = np.where(live, fm, np.float32(0)).astype(np.float32)
            ce = np.where(live, be + pe[t][z[sl]] + fe, ZERO_E)
            if drop is not None and live.any():
                top = np.lexsort((cm, ce))[-1]
                cut = int(round(math.log2(drop)))
                assert 2.0 ** cut == drop
                gone = live & _gt(cm[top], ce[top] + cut, cm, ce)
                cm, ce = np.where(gone, np.float32(0), cm).astype(np.float32), np.where(gone, ZERO_E, ce)
            nm[lo + 2:hi + 3], ne[lo + 2:hi + 3] = cm, ce
            bp[t, sl] = arg
        am, ae = nm, ne
    c0 = (am[2 * L + 2], ae[2 * L + 2])
    c1 = (am[2 * L + 1], ae[2 * L + 1]) if L else (np.float32(0), ZERO_E)
    end, best = (2 * L - 1, c1) if _gt(c1[0], c1[1], c0[0], c0[1]) else (2 * L, c0)
    if not best[0] > 0:
        return dict(none, logp=-math.inf)
    logp = math.log(float(best[0])) + int(best[1]) * math.log(2.0)
    states = [0] * T
    s = end
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    assert s == 0 and states[0] in (0, 1)
    start, count = spans(states, L)
    qual = []
    for k in range(L):
        tot = p[start[k], y[k]]
        for j in range(1, count[k]):
            tot = np.float32(tot + p[start[k] + j, y[k]])
        qual.append(np.float32(tot / np.float32(count[k])))
    return dict(logp=logp, start=start, count=count, qual=qual, states=states)


def spans(states, L):
    """(start, count) of every label's state 2k + 1 in a state sequence"""
    start, count = [None] * L, [0] * L
    for t, s in enumerate(states):
        if s & 1:
            if count[s >> 1] == 0:
                start[s >> 1] = t
            count[s >> 1] += 1
    return start, count


def enumerate_alignments(p, y, collapse_repeats=True):
    """every state sequence of labelling y over the T rows of p with its float64 probability, best first"""
    p = np.asarray(p, np.float64)
    T = p.shape[0]
    L = len(y)
    z = [0] * (2 * L + 1)
    z[1::2] = [int(v) for v in y]
    out = []

    def step(seq, w):
        if len(seq) == T:
            if seq[-1] in (2 * L, 2 * L - 1):
                out.append((w, tuple(seq)))
            return
        s = seq[-1]
        nxt = []
        if not (s & 1) or collapse_repeats:
            nxt.append(s)
        if s + 1 <= 2 * L:
            nxt.append(s + 1)
        if s + 2 <= 2 * L and (s + 2) & 1 and (not collapse_repeats or z[s + 2] != z[s]):
            nxt.append(s + 2)
        for n in nxt:
            step(seq + [n], w * p[len(seq), z[n]])
    for s0 in ((0, 1) if L else (0,)):
        if T:
            step([s0], p[0, z[s0]])
    out.sort(key=lambda a: -a[0])
    return out
