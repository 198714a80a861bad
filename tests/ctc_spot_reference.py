"""TEST INFRASTRUCTURE: CTC motif spotting as include/fcd.h defines it (fcd_ctc_spot_*) in plain float64 numpy.  A cell's
candidates are stacked in the order stay, s-1, s-2, so argmax (the first maximum) is the definition's tie rule.  The kernels
round every cell to f32, this does not: `margin` (the smallest ratio by which the best end row beats another and the winner
the best loser at a cell of the best path), `floor` (the smallest non-zero cell) and `tied` say whether the two can differ
in a decision.  Where they cannot, v_hit is exactly the f32 product along the path in row order: `logp` is formed from it."""
import math

import numpy as np

from ctc_align_reference import spans


def ctc_spot(p, y, collapse_repeats=True, b=0, e=None):
    """p: (T, N) float32, y: labels, rows [b, e) -> dict(logp, end, start, count, qual, track (float64 ln v_t, one a row of
    the range), margin, floor, tied); end None where there is no hit"""
    b, e, _ = slice(b, e).indices(p.shape[0])
    y, x = [int(v) for v in y], p[b:e].astype(np.float64)
    L, rows = len(y), max(e - b, 0)
    none = dict(end=None, track=None, margin=math.inf, floor=math.inf, tied=False)
    if any(not 1 <= v < p.shape[1] for v in y):
        return dict(none, logp=math.nan)
    if L == 0 or L > rows:
        return dict(none, logp=0.0 if L == 0 else -math.inf)
    if not (np.isfinite(x).all() and (x >= 0).all()):
        return dict(none, logp=math.nan)
    S = 2 * L  # states 0 .. 2L - 1: state 0 is pinned to 1, 2L plays no part
    z = np.zeros(S, np.int64)
    z[1::2] = y
    odd = np.arange(S) % 2 == 1
    skip = odd & (np.arange(S) >= 3) & ((z != np.roll(z, 2)) | (not collapse_repeats))
    a, cells, cands = np.eye(1, S)[0], [], []
    for t in range(rows):  # (-1: not a candidate; what has no path yet is 0, so s <= 2 (t - b) + 1 holds by itself)
        c = np.stack([np.where(odd & (not collapse_repeats), -1.0, a), np.roll(a, 1), np.where(skip, np.roll(a, 2), -1.0)])
        a = c.max(0) * x[t, z]
        a[0] = 1.0
        cells.append(a)
        cands.append(c)
    cells = np.array(cells)
    track = cells[:, -1]
    with np.errstate(divide="ignore"):
        out = dict(none, logp=-math.inf, track=np.log(track), floor=cells[cells > 0].min())
    if not track.max() > 0:
        return out
    end = int(np.argmax(track))  # (the first of equal maxima)
    rest = np.delete(track, end).max(initial=0.0)
    margin, tied, states, s, t = (track[end] / rest if rest > 0 else math.inf), rest == track[end], [], S - 1, end
    while s > 0:
        states.append(s)
        win, lose = np.sort(cands[t][:, s])[:0:-1]
        margin, tied = (min(margin, win / lose) if lose > 0 else margin), tied or (win == lose and win > 0)
        s, t = s - int(np.argmax(cands[t][:, s])), t - 1
    states.reverse()
    first = b + t + 1  # the hit's first row
    start, count = spans(states, L)
    start = [first + v for v in start]
    m, ex = np.float32(0.5), 1  # the f32 product along the path: mantissa and exponent
    for i, s in enumerate(states):
        pm, pe = np.frexp(p[first + i, z[s]])
        m, e2 = np.frexp(np.float32(m * pm))
        ex += int(pe) + int(e2)
    qual = [np.float32(np.add.accumulate(p[start[k]:start[k] + count[k], y[k]], dtype=np.float32)[-1] / np.float32(count[k]))
            for k in range(L)]
    return dict(out, logp=math.log(float(m)) + ex * math.log(2.0), end=first + len(states) - 1, start=start, count=count,
                qual=qual, margin=margin, tied=bool(tied))
