"""TEST INFRASTRUCTURE: CTC motif occurrence posteriors as include/fcd.h defines them (fcd_ctc_detect_*), a plain float64
loop, and what they stand for by brute force: the expected number of occurrences of a motif over all N^T paths."""
import itertools
import math

import numpy as np


def ctc_detect(p, y, collapse=True, b=0, e=None):
    """p: (T, N) f32, rows [b, e) -> dict(count, end (absolute row or None), logp, c (float64 c_t of the range, or None))"""
    b, e, _ = slice(b, e).indices(p.shape[0])
    y, x = [int(v) for v in y], p[b:e].astype(np.float64)
    L, rows, nan = len(y), max(e - b, 0), math.nan
    walks = 0 < L <= rows
    if any(not 1 <= v < p.shape[1] for v in y) or (walks and not (np.isfinite(x).all() and (x >= 0).all())):
        return dict(end=None, c=None, logp=nan, count=nan)
    if not walks:
        return dict(end=None, c=None, logp=0.0 if L == 0 else -math.inf, count=0.0)
    a, c = [0.0] * (2 * L), []  # states 1 .. 2L - 1; a[0] is never a cell
    for t in range(rows):
        g = 1.0 if t == 0 or not collapse else max(0.0, 1.0 - x[t - 1, y[0]])
        new = [0.0] * (2 * L)
        for s in range(1, 2 * L):
            k, total = s >> 1, (a[s] if collapse or not s & 1 else 0.0) + (g if s == 1 else a[s - 1])
            if s & 1 and s >= 3 and (not collapse or y[k] != y[k - 1]):
                total += a[s - 2]
            new[s] = total * x[t, y[k] if s & 1 else 0]
        a = new
        c.append(a[2 * L - 1] * (1.0 if t == rows - 1 or not collapse else max(0.0, 1.0 - x[t + 1, y[-1]])))
    if not max(c) > 0:
        return dict(end=None, c=c, logp=-math.inf, count=0.0)
    end = int(np.argmax(c))  # (the first of equal maxima)
    return dict(end=b + end, c=c, logp=math.log(c[end]), count=math.fsum(c))


def expected_count(p, y, collapse=True):
    """sum over all N^T paths of P(path) * #{occurrences of y in the path's labelling, overlaps included}; rows sum to 1"""
    x, y, total = p.astype(np.float64), [int(v) for v in y], 0.0
    for path in itertools.product(range(p.shape[1]), repeat=p.shape[0]):
        lab = [v for i, v in enumerate(path) if v and not (collapse and i and path[i - 1] == v)]
        n = sum(lab[i:i + len(y)] == y for i in range(len(lab) - len(y) + 1))
        total += n * math.prod(x[t, v] for t, v in enumerate(path)) if n else 0.0
    return total
