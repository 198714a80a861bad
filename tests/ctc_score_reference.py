"""TEST INFRASTRUCTURE: the CTC forward log-likelihood fcd_ctc_score_* computes (include/fcd.h), restated in float64
numpy straight from its definition -- the specification the kernel (csrc/ctc_score.hip) is held to -- and a brute-force
enumerator that sums the product of the posteriors over every alignment of a tiny case.

Extended sequence z of 2L + 1 states (z[2k] = blank, z[2k+1] = y[k]):
    start   alpha_0[0] = p[0][0], alpha_0[1] = p[0][y_0]
    blank   alpha_t[s] = (alpha_{t-1}[s] + alpha_{t-1}[s-1]) p[t][0]
    label   collapse:     (alpha_{t-1}[s] + alpha_{t-1}[s-1] + [s >= 3, z[s] != z[s-2]] alpha_{t-1}[s-2]) p[t][z[s]]
            no collapse:  (alpha_{t-1}[s-1] + [s >= 3] alpha_{t-1}[s-2]) p[t][z[s]]
    result  ln(alpha_{T-1}[2L] + alpha_{T-1}[2L-1])
band = W >= 1: with k(t) = #{k : path[k] <= t}, states outside max(0, 2(k(t)-W)-2) .. min(2L, 2(k(t)+W)) count as 0 at row t.
Rows are rescaled by exact powers of two (an integer exponent total), so that T = 4000 does not underflow float64."""
import bisect
import itertools
import math

import numpy as np


def ctc_logp(p, y, collapse_repeats=True, band=0, path=None, drop=None):
    """p: (T, N) posteriors (any float type; used as float64), y: label indices 1 .. N-1 -> ln P(y | p) as a float.
    drop: cells below drop * (the row's largest live cell) are zeroed -- what the contract lets the kernel lose."""
    p = np.asarray(p, np.float64)
    T, N = p.shape
    y = [int(v) for v in y]
    L = len(y)
    if any(not 1 <= v < N for v in y):
        return math.nan
    if T == 0:
        return 0.0 if L == 0 else -math.inf
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
    ap = np.zeros(S + 2)  # ap[s + 2] = alpha[s]: two zeros in front stand for the states below 0
    total_exp = 0
    with np.errstate(all="ignore"):
        for t in range(T):
            lo, hi = 0, 2 * L
            if band:
                k = bisect.bisect_right(path, t)
                lo, hi = max(0, 2 * (k - band) - 2), min(2 * L, 2 * (k + band))
            nxt = np.zeros(S + 2)  # (every state outside lo .. hi counts as 0 at this row)
            if hi >= lo:
                pz = p[t][z[lo:hi + 1]]
                if t == 0:
                    new = np.zeros(hi - lo + 1)
                    new[:2 - lo] = pz[:2 - lo] if lo < 2 else 0.0
                else:
                    a0, a1, a2 = ap[lo + 2:hi + 3], ap[lo + 1:hi + 2], ap[lo:hi + 1]
                    s2 = np.where(skip[lo:hi + 1], a2, 0.0)
                    if collapse_repeats:
                        tot = a0 + a1 + s2
                    else:
                        tot = np.where(odd[lo:hi + 1], a1 + s2, a0 + a1)
                    new = tot * pz
                fin = new[np.isfinite(new)]
                m = fin.max() if fin.size else 0.0
                if m > 0.0:
                    e = math.frexp(m)[1]
                    new = np.ldexp(new, -e)
                    total_exp += e
                    if drop is not None:
                        new[new < drop * math.ldexp(m, -e)] = 0.0
                nxt[lo + 2:hi + 3] = new
            ap = nxt
        a = ap[2:]
        P = a[2 * L] + (a[2 * L - 1] if L > 0 else 0.0)
        if P != P:
            return math.nan
        if P <= 0.0:
            return -math.inf if P == 0.0 else math.nan
        return math.log(P) + total_exp * math.log(2.0)


def collapse_alignment(pi, collapse_repeats):
    """the labelling an alignment (one symbol per row, 0 = blank) spells"""
    out = []
    prev = 0
    for c in pi:
        if c != 0 and not (collapse_repeats and c == prev):
            out.append(c)
        prev = c
    return tuple(out)


def enumerate_all(p, collapse_repeats=True):
    """p: (T, N) -> {labelling: sum over its alignments of prod_t p[t][pi_t]}, every labelling with an alignment"""
    p = np.asarray(p, np.float64)
    T, N = p.shape
    out = {}
    for pi in itertools.product(range(N), repeat=T):
        w = 1.0
        for t, c in enumerate(pi):
            w *= p[t, c]
        key = collapse_alignment(pi, collapse_repeats)
        out[key] = out.get(key, 0.0) + w
    return out
