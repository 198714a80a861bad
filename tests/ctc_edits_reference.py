"""TEST INFRASTRUCTURE: the deletion and insertion likelihoods fcd_ctc_edits_* computes (include/fcd.h), restated in
float64 twice.

ctc_edits_rescored: exact mode straight from what the numbers mean -- ln P(y without label k | p) and ln P(y with c
inserted at gap g | p), every one a full scoring of the variant labelling with tests/ctc_score_reference.py::ctc_logp.
No forward-backward.

ctc_edits_dense: the definition of include/fcd.h, word for word, on dense alpha / b arrays (one row per row of the read,
one column per state, the band's window as a mask): what the numbers are under a band, where a variant has no window of
its own to be rescored in.  No slots, no shared scales, no reachability cuts: nothing of the kernel's bookkeeping.  Rows
are rescaled by powers of two with integer exponents so that long reads stay inside float64.

Both return (deletion (L,), insertion (L + 1, N - 1), logp): log-ratios against ln P(y | p); all NaN when that is not a
finite number."""
import bisect
import math

import numpy as np

import ctc_score_reference as R


def _ratio(v, logp):
    if v != v:
        return math.nan
    return v - logp  # (-inf stays -inf)


def ctc_edits_rescored(p, y, collapse_repeats=True):
    p = np.asarray(p, np.float64)
    N = p.shape[1]
    y = [int(v) for v in y]
    L = len(y)
    logp = R.ctc_logp(p, y, collapse_repeats)
    dele = np.full(L, math.nan)
    ins = np.full((L + 1, N - 1), math.nan)
    if not math.isfinite(logp):
        return dele, ins, logp
    for k in range(L):
        dele[k] = _ratio(R.ctc_logp(p, y[:k] + y[k + 1:], collapse_repeats), logp)
    for g in range(L + 1):
        for c in range(1, N):
            ins[g, c - 1] = _ratio(R.ctc_logp(p, y[:g] + [c] + y[g:], collapse_repeats), logp)
    return dele, ins, logp


def _norm(row):
    """row / 2^e with its largest finite entry in [0.5, 1) -> (row, e)"""
    fin = row[np.isfinite(row)]
    m = fin.max() if fin.size else 0.0
    if m > 0.0:
        e = math.frexp(m)[1]
        return np.ldexp(row, -e), e
    return row, 0


def _log_sum(terms):
    """ln of the sum of m * 2^e over (m, e); NaN if any m is NaN, -inf for an empty or all-zero sum"""
    terms = [(m, e) for m, e in terms if m != 0.0]
    if any(m != m for m, _ in terms):
        return math.nan
    if not terms:
        return -math.inf
    big = max(e for _, e in terms)
    tot = sum(math.ldexp(m, max(e - big, -4000)) for m, e in terms)
    return math.log(tot) + big * math.log(2.0)


def ctc_edits_dense(p, y, collapse_repeats=True, band=0, path=None):
    p = np.asarray(p, np.float64)
    T, N = p.shape
    y = [int(v) for v in y]
    L = len(y)
    logp = R.ctc_logp(p, y, collapse_repeats, band, path)
    dele = np.full(L, math.nan)
    ins = np.full((L + 1, N - 1), math.nan)
    if not math.isfinite(logp):
        return dele, ins, logp
    S = 2 * L + 1
    z = np.zeros(S, np.int64)
    z[1::2] = y
    col = bool(collapse_repeats)
    live = np.ones((T, S), bool)
    if band:
        pth = [int(v) for v in path]
        for t in range(T):
            k = bisect.bisect_right(pth, t)
            lo, hi = max(0, 2 * (k - band) - 2), min(2 * L, 2 * (k + band))
            live[t] = False
            live[t, lo:hi + 1] = True
    with np.errstate(all="ignore"):
        # alpha[t + 1] = alpha_t (alpha[0]: "row -1", all mass on state 0), true value alpha * 2^ea
        alpha = np.zeros((T + 1, S + 2))  # [.., s + 2]: two zeros in front stand for the states below 0
        ea = np.zeros(T + 1, np.int64)
        alpha[0, 2] = 1.0
        for t in range(T):
            a = alpha[t]
            new = np.zeros(S)
            for s in range(S):
                if not live[t, s]:
                    continue
                tot = a[s + 1]
                if s % 2 == 0 or col:
                    tot = tot + a[s + 2]
                if s % 2 == 1 and s >= 3 and (not col or z[s] != z[s - 2]):
                    tot = tot + a[s]
                new[s] = tot * p[t, z[s]]
            new, e = _norm(new)
            alpha[t + 1, 2:] = new
            ea[t + 1] = ea[t] + e
        # b[t] = b_t (b[T]: "row T", all mass on state 2L), true value b * 2^eb; u[t][g][c - 1] shares b's scale
        b = np.zeros((T + 1, S + 2))  # two zeros behind stand for the states above 2L
        eb = np.zeros(T + 1, np.int64)
        b[T, 2 * L] = 1.0
        u = np.zeros((T + 1, L + 1, N - 1))
        for t in range(T - 1, -1, -1):
            nb = b[t + 1]
            new = np.zeros(S)
            for s in range(S):
                if not live[t, s]:
                    continue
                tot = nb[s + 1]
                if s % 2 == 0 or col:
                    tot = tot + nb[s]
                if s % 2 == 1 and s + 2 < S and (not col or z[s + 2] != z[s]):
                    tot = tot + nb[s + 2]
                new[s] = tot * p[t, z[s]]
            for g in range(L + 1):
                if not live[t, 2 * g]:
                    continue
                for c in range(1, N):
                    tot = nb[2 * g]
                    if col:
                        tot = tot + u[t + 1, g, c - 1]
                    if g < L and (not col or c != y[g]):
                        tot = tot + nb[2 * g + 1]
                    u[t, g, c - 1] = tot * p[t, c]
            both = np.concatenate([new, u[t].ravel()])
            _, e = _norm(both)
            b[t, :S] = np.ldexp(new, -e)
            u[t] = np.ldexp(u[t], -e)
            eb[t] = eb[t + 1] + e
        for k in range(L):
            if k == L - 1:
                if live[T - 1, 2 * L - 1]:
                    a = alpha[T]
                    v = a[2 * L - 2 + 2] + (a[2 * L - 3 + 2] if L >= 2 else 0.0)
                    dele[k] = _ratio(_log_sum([(v, int(ea[T]))]), logp)
                else:
                    dele[k] = -math.inf
                continue
            terms = []
            for t in range(T):
                if not live[t, 2 * k + 1]:
                    continue
                a = alpha[t]
                entry = a[2 * k + 2]
                if k >= 1 and (not col or y[k - 1] != y[k + 1]):
                    entry = entry + a[2 * k - 1 + 2]
                terms.append((entry * b[t, 2 * k + 3], int(ea[t] + eb[t])))
            dele[k] = _ratio(_log_sum(terms), logp)
        for g in range(L + 1):
            for c in range(1, N):
                terms = []
                for t in range(T):
                    if not live[t, 2 * g]:
                        continue
                    a = alpha[t]
                    entry = a[2 * g + 2]
                    if g >= 1 and (not col or c != y[g - 1]):
                        entry = entry + a[2 * g - 1 + 2]
                    terms.append((entry * u[t, g, c - 1], int(ea[t] + eb[t])))
                ins[g, c - 1] = _ratio(_log_sum(terms), logp)
    return dele, ins, logp


def ctc_edits(p, y, collapse_repeats=True, band=0, path=None):
    """what the kernel is held to: the rescoring restatement in exact mode, the dense one under a band"""
    if band:
        return ctc_edits_dense(p, y, collapse_repeats, band, path)
    return ctc_edits_rescored(p, y, collapse_repeats)
