"""TEST INFRASTRUCTURE: CRF motif occurrence posteriors as include/fcd.h defines them (fcd_crf_detect_*), a plain float64
loop, and what they stand for by brute force: the expected number of occurrences of a motif over every start state and
symbol sequence of a tiny case, under the path measure fcd_crf_marginals_* defines."""
import math

import numpy as np

import crf_transitions_reference as TR


def history(S, N):
    """m of S = (N - 1)^m; S = 1 walks as m = 1"""
    nb, m, v = N - 1, 0, 1
    while v < S:
        v, m = v * nb, m + 1
    assert v == S, "S must be a power of N - 1"
    return max(m, 1)


def crf_detect(p, marg, y, b=0, e=None):
    """p, marg: (T, S, N), rows [b, e) -> dict(count, end (absolute row or None), logp, c (float64 c_u of the range, or None))"""
    T, S, N = p.shape
    b, e, _ = slice(b, e).indices(T)
    y, nb, m, nan = [int(v) for v in y], N - 1, history(S, N), math.nan
    L = len(y)
    if any(not 1 <= v < N for v in y):
        return dict(end=None, c=None, logp=nan, count=nan)
    if L == 0 or e <= b:
        return dict(end=None, c=None, logp=0.0 if L == 0 else -math.inf, count=0.0)
    x, g = p[b:e].astype(np.float64), marg[b:e].astype(np.float64)
    h = min(L, m)
    prefix = 0
    for v in y[:h - 1]:
        prefix = prefix * nb + v - 1
    entry = [s for s in range(prefix, S, nb ** (h - 1))]  # ascending: d * nb^(h-1) + prefix
    sigma = {}
    for k in range(h, L):  # (k >= m: the m labels behind cell k exist)
        s = 0
        for v in y[k - m:k]:
            s = s * nb + v - 1
        sigma[k] = s
    live = [k for k in range(h, L) if sigma[k] < S]  # (a state outside the table reads 0 and is never looked at)
    read = [g[:, entry, y[h - 1]]] + [x[:, sigma[k], 0] for k in live] + [x[:, sigma[k], y[k]] for k in live]
    if any(not (np.isfinite(v).all() and (v >= 0).all()) for v in read):
        return dict(end=None, c=None, logp=nan, count=nan)
    a, c = {k: 0.0 for k in range(h, L)}, []
    for u in range(e - b):
        e_u = 0.0
        for s in entry:
            e_u += g[u, s, y[h - 1]]
        post = lambda k, j: x[u, sigma[k], j] if sigma[k] < S else 0.0  # noqa: E731
        c.append(a[L - 1] * post(L - 1, y[L - 1]) if L > h else e_u)
        a = {k: a[k] * post(k, 0) + (e_u if k == h else a[k - 1] * post(k - 1, y[k - 1])) for k in range(h, L)}
    if not max(c) > 0:
        return dict(end=None, c=c, logp=-math.inf, count=0.0)
    end, count = int(np.argmax(c)), 0.0  # (the first of equal maxima)
    for v in c:
        count += v  # (in row order)
    return dict(end=b + end, c=c, logp=math.log(c[end]), count=count)


def expected_count(scores, y):
    """sum over every (start state, symbol sequence) of P(path) * #{occurrences of y in the start state's m labels followed by
    the emitted ones, overlaps included, whose min(L, m)-th label is an emitted one}"""
    T, S, N = scores.shape
    nb, m, y = N - 1, history(S, N), [int(v) for v in y]
    h, paths = min(len(y), m), TR.enumerate_paths(scores)
    top = max(q[3] for q in paths)
    total = z = 0.0
    for s0, sym, _, score in paths:
        w = math.exp(score - top)
        z += w
        lab = [s0 // nb ** (m - 1 - j) % nb + 1 for j in range(m)] + [a for a in sym if a]
        total += w * sum(lab[i:i + len(y)] == y and i + h - 1 >= m for i in range(len(lab) - len(y) + 1))
    return total / z
