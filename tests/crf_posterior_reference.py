"""TEST INFRASTRUCTURE: what fcd_crf_posterior_* computes (include/fcd.h), restated in float64 straight from the
definition -- the specification the kernels (csrc/crf_posterior.hip) are held to.  No backward walk and no closed-form
trajectory here: every variant y[k:=c] is scored on its own by tests/crf_lattice_reference.crf_score, its trajectory
computed from scratch, under a band with the window of y's OWN path (windows are in label counts, so the path array of y
serves the variant as it is)."""
import math

import numpy as np

import crf_lattice_reference as R


def crf_substitutions(p, init, y, band=0, path=None):
    """-> (sub_ln (L, N-1) float64: ln P(y[k:=c] | x), -inf for none, NaN where a NaN enters; logp = crf_score(y))"""
    p = np.asarray(p)
    N = p.shape[2]
    y = [int(v) for v in y]
    L = len(y)
    logp = R.crf_score(p, init, y, band, path)
    sub = np.full((L, N - 1), math.nan)
    if logp != logp or any(not 1 <= v < N for v in y):
        return sub, logp
    for k in range(L):
        for c in range(1, N):
            sub[k, c - 1] = logp if c == y[k] else R.crf_score(p, init, y[:k] + [c] + y[k + 1:], band, path)
    return sub, logp


def crf_posterior(p, init, y, band=0, path=None):
    """-> (post (L, N-1) float64, logp).  Every entry NaN where P(y | x) is not a positive finite number; a position whose
    sum over c is 0 or NaN is NaN."""
    sub, logp = crf_substitutions(p, init, y, band, path)
    post = np.full(sub.shape, math.nan)
    if not math.isfinite(logp):
        return post, logp
    for k in range(sub.shape[0]):
        row = sub[k]
        if np.isnan(row).any():
            continue
        top = row.max()
        if top == -math.inf:
            continue
        w = np.exp(row - top)  # (the largest entry is 1: the sum is positive and finite)
        post[k] = w / w.sum()
    return post, logp
