"""TEST INFRASTRUCTURE: CRF motif spotting as include/fcd.h defines it (fcd_crf_spot_*), a plain float64 loop with stacked
candidates (stay first) and first-maximum argmax, and what it stands for by brute force on a tiny case: the maximum over
every entry row and every run of stays and emissions, enumerated outright.  `margin` is the smallest ratio by which the best
end row beats another and a winner the loser at a cell of the best path: where it is well above 1 the f32 kernel takes the
same decisions."""
import math

import numpy as np

from crf_detect_reference import history


def _setup(p, marg, y, b, e):
    T, S, N = p.shape
    b, e, _ = slice(b, e).indices(T)
    y, nb, m = [int(v) for v in y], N - 1, history(S, N)
    L, h = len(y), min(len(y), m)
    prefix = 0
    for v in y[:max(h - 1, 0)]:
        prefix = prefix * nb + v - 1
    entry = list(range(prefix, S, nb ** max(h - 1, 0)))  # ascending
    sigma = {}
    for k in range(h, L):
        s = 0
        for v in y[k - m:k]:
            s = s * nb + v - 1
        sigma[k] = s
    return b, e, y, L, h, entry, sigma


def crf_spot(p, marg, y, b=0, e=None):
    """p, marg: (T, S, N), rows [b, e) -> dict(logp, end, first, start (absolute emission rows of labels h - 1 .. L - 1), v
    (float64 v_u of the range, or None), e_first, margin); end None where there is no hit"""
    S, N = p.shape[1:]
    b, e, y, L, h, entry, sigma = _setup(p, marg, y, b, e)
    none = dict(end=None, v=None, margin=math.inf)
    if any(not 1 <= v < N for v in y):
        return dict(none, logp=math.nan)
    if L == 0 or e <= b:
        return dict(none, logp=0.0 if L == 0 else -math.inf)
    x, g = p[b:e].astype(np.float64), marg[b:e].astype(np.float64)
    live = [k for k in range(h, L) if sigma[k] < S]
    read = [g[:, entry, y[h - 1]]] + [x[:, sigma[k], 0] for k in live] + [x[:, sigma[k], y[k]] for k in live]
    if any(not (np.isfinite(v).all() and (v >= 0).all()) for v in read):
        return dict(none, logp=math.nan)
    post = lambda u, k, j: x[u, sigma[k], j] if sigma[k] < S else 0.0  # noqa: E731
    a, v, ups, cands, ent = {k: 0.0 for k in range(h, L)}, [], [], [], []
    for u in range(e - b):
        e_u = 0.0
        for s in entry:
            e_u += g[u, s, y[h - 1]]
        ent.append(e_u)
        v.append(a[L - 1] * post(u, L - 1, y[L - 1]) if L > h else e_u)
        c = {k: (a[k] * post(u, k, 0), e_u if k == h else a[k - 1] * post(u, k - 1, y[k - 1])) for k in range(h, L)}
        ups.append({k: int(np.argmax(c[k])) for k in c})  # (the first maximum: stay unless strictly greater)
        cands.append(c)
        a = {k: max(c[k]) for k in c}
    if not max(v) > 0:
        return dict(none, v=v, logp=-math.inf)
    end = int(np.argmax(v))
    rest = max(v[:end] + v[end + 1:], default=0.0)
    margin = v[end] / rest if rest > 0 else math.inf
    start, k, u = [end], L - 1, end - 1
    while k >= h:  # cell k at row u: entered here, or stayed
        win, lose = sorted(cands[u][k])[::-1]
        margin = min(margin, win / lose) if lose > 0 else margin
        if ups[u][k]:
            start.append(u)
            k -= 1
        u -= 1
    start = [b + t for t in reversed(start)] if L > h else [b + end]
    first = start[0]
    e_first = np.float32(0)
    for s in entry:  # (the kernel's own sum: f32, ascending)
        e_first = np.float32(e_first + marg[first, s, y[h - 1]])
    return dict(logp=math.log(v[end]), end=b + end, first=first, start=start, v=v, e_first=e_first, margin=margin,
                h=h, sigma=sigma)


def brute_force(p, marg, y):
    """max over the entry row u0 and every run of stays and emissions behind it, of the product of its weights"""
    b, e, y, L, h, entry, sigma = _setup(p, marg, y, 0, None)
    x, g = p.astype(np.float64), marg.astype(np.float64)

    def best(u, k, w):  # in cell k after row u - 1 with weight w: the best completion
        if k == L:
            return w
        if u == e:
            return 0.0
        return max(best(u + 1, k, w * x[u, sigma[k], 0]), best(u + 1, k + 1, w * x[u, sigma[k], y[k]]))
    return max(best(u0 + 1, h, sum(g[u0, s, y[h - 1]] for s in entry)) for u0 in range(e))
