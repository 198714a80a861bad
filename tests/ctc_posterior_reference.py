"""TEST INFRASTRUCTURE: the substitution posteriors fcd_ctc_posterior_* computes (include/fcd.h), restated in float64
straight from their definition -- post[k][c] = P(y[k:=c] | x) / sum_c' P(y[k:=c'] | x), every P the CTC forward
log-likelihood tests/ctc_score_reference.py::ctc_logp of the variant labelling, under a band the window of y's OWN path.
No forward-backward shortcut: L * (N - 1) full scorings.  The specification the kernel (csrc/ctc_posterior.hip) is held to."""
import math

import numpy as np

import ctc_score_reference as R


def ctc_sub_logp(p, y, collapse_repeats=True, band=0, path=None):
    """-> (L, N - 1) float64: ln P(y[k:=c] | p) for every position k and label c = 1 .. N-1"""
    p = np.asarray(p, np.float64)
    N = p.shape[1]
    y = [int(v) for v in y]
    out = np.empty((len(y), N - 1))
    for k in range(len(y)):
        for c in range(1, N):
            out[k, c - 1] = R.ctc_logp(p, y[:k] + [c] + y[k + 1:], collapse_repeats, band, path)
    return out


def ctc_posterior(p, y, collapse_repeats=True, band=0, path=None):
    """-> (post (L, N - 1) float64, logp): NaN everywhere when P(y | p) is not positive and finite; a position whose sum
    over c is 0 or NaN is NaN"""
    p = np.asarray(p, np.float64)
    N = p.shape[1]
    logp = R.ctc_logp(p, y, collapse_repeats, band, path)
    post = np.full((len(y), N - 1), math.nan)
    if not math.isfinite(logp):
        return post, logp
    sub = ctc_sub_logp(p, y, collapse_repeats, band, path)
    for k in range(len(y)):
        row = sub[k]
        if np.isnan(row).any() or not np.isfinite(row.max()):
            continue
        e = np.exp(row - row.max())  # (the largest term is 1: no underflow of the sum)
        post[k] = e / e.sum()
    return post, logp
