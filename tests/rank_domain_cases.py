"""TEST INFRASTRUCTURE: constructed inputs for the f32 rank count of the headline beam kernels (csrc/device_utils.h,
FCD_RANKF4: two reads per wavefront, reads of one length, N = 3, 4, 5).  The count is exact while every candidate word of a
half is that of +0 or of a finite probability in [2^-76, 2^27]; a step that holds any other candidate is sent to the exact
recount by a wave-wide vote (fcd_rankf_outside).  Shared by tests/test_rank_domain_emu.py (CPU, emulated kernels) and
tests/test_gpu_rank_domain.py; the runners are those of tests/rank32_cases.py.

Every read is compared with the oracle: status, out_len, labels, path -- under both tie orders, beams 5 and 3.
Launches of 2 .. 8 reads, T <= 48 (tables INSIDE, OUTSIDE, HALVES):
  inside the domain on every step: plain random rows; ties there (quantised, two equal columns, constant rows); a first row
    that holds 2^-76 and its upper neighbour, and one that holds 2^27;
  outside it, alone and mixed with in-domain candidates of the same half: rows scaled by 2^-80 and subnormal rows under
    threshold 0; one column scaled by 2^-80; rows scaled by 2^30, one column scaled by 2^30 or 2^40, a +inf; negative posteriors
    (threshold -1); a first row that holds the lower neighbour of 2^-76, and one that holds the upper neighbour of 2^27; the lone NaNs,
    the NaN among several and the empty list of rank32_cases.failing_launches();
  exact +0 candidates among in-domain ones, and the zeros of both signs of rank32_cases.zero_cols: inside (the word of +0
    is part of the domain, and -0.0 ranks as +0);
  one wavefront with its first half inside and its second half outside, and the reverse.
outside_steps() follows the reference's search (tests/naive_reference.py) and says, per step, whether a candidate of the
step is outside the domain: the CPU test asserts from it that each case enters or avoids the guard as it is named."""
import numpy as np

import naive_reference as NV
import rank32_cases as RC

N = RC.N
T = RC.T
BEAMS = RC.BEAMS
P_LO = np.float32(2.0 ** -76)
P_HI = np.float32(2.0 ** 27)


def in_domain(p):
    """a candidate probability whose word the f32 count is exact on: +0 (make_key turns -0.0 into it) or [2^-76, 2^27]"""
    p = float(p)
    return p == 0.0 or (float(P_LO) <= p <= float(P_HI))


def outside_steps(x, beam, thr, collapse=True):
    """per step of the reference's search: does the merged candidate list hold a probability outside the domain?
    Stops behind the step that fails (a NaN among several, an empty list): that step still ranks."""
    x = np.asarray(x, np.float32)
    n = x.shape[1]
    thr = NV.f32(thr)
    rows = [[float(v) for v in r] for r in x]
    tree = NV.SuffixTree(n - 1)
    cur = [NV.Point1(NV.ROOT_NODE, 0, 0.0, 1.0)]
    steps = []
    for idx, pr in enumerate(rows):
        nxt = []
        for b in cur:
            tip = tree.label(b.node)
            if pr[0] > thr:
                nxt.append(NV.Point1(b.node, 0, 0.0, NV.f32(NV.f32(b.label_prob + b.gap_prob) * pr[0])))
            for label in range(n - 1):
                pb = pr[label + 1]
                if pb < thr:
                    continue
                if collapse and label == tip:
                    nxt.append(NV.Point1(b.node, 0, NV.f32(b.label_prob * pb), 0.0))
                    nn = tree.get_child(b.node, label)
                    if nn is None and b.gap_prob > 0.0:
                        nn = tree.add_node(b.node, label, idx)
                    if nn is not None:
                        nxt.append(NV.Point1(nn, 0, NV.f32(b.gap_prob * pb), 0.0))
                else:
                    nn = tree.get_child(b.node, label)
                    if nn is None:
                        nn = tree.add_node(b.node, label, idx)
                    nxt.append(NV.Point1(nn, 0, NV.f32(NV.f32(b.label_prob + b.gap_prob) * pb), 0.0))
        merged = []
        for item in NV.stable_sort_by_node(nxt):
            if merged and merged[-1].node == item.node:
                merged[-1].label_prob = NV.f32(merged[-1].label_prob + item.label_prob)
                merged[-1].gap_prob = NV.f32(merged[-1].gap_prob + item.gap_prob)
            else:
                merged.append(item)
        steps.append(any(not in_domain(c.probability()) for c in merged))
        try:
            srt = NV.sort_by_probability_desc(merged, NV.Point1.probability)
        except NV.SearchError:
            break
        if not srt:
            break
        cur = srt[:beam]
        top = cur[0].probability()
        for c in cur:
            c.label_prob = NV.f32_div(c.label_prob, top)
            c.gap_prob = NV.f32_div(c.gap_prob, top)
    return steps


def mixed_steps(x, beam, thr):
    """steps that hold a candidate outside the domain AND a positive one inside it (same half): the guard must not depend
    on who else is there -- counted from the first row alone, where the candidates are the row's own values"""
    r0 = [float(v) for v in np.asarray(x, np.float32)[0]]
    cand = [v for j, v in enumerate(r0) if (v > thr if j == 0 else not v < thr)]
    return any(not in_domain(v) for v in cand) and any(in_domain(v) and v > 0.0 for v in cand)


# ---- reads ----------------------------------------------------------------------------------------------------------
def scaled(seed, e, T=T, n=N):
    """plain random rows times 2^e (a power of two: every product and quotient of the search scales exactly, except where
    it leaves the normal range)"""
    x = np.random.default_rng(seed).random((T, n), dtype=np.float32)
    x /= x.sum(-1, keepdims=True)
    return (x * np.float32(2.0 ** e)).astype(np.float32)


def one_column(seed, e, col=3, T=T):
    """plain random rows whose column `col` alone is scaled by 2^e: its children leave the domain, their siblings stay"""
    x = RC.plain_random(seed, T)
    x[:, col] *= np.float32(2.0 ** e)
    return x.astype(np.float32)


def with_inf(seed, col, T=12):
    x = RC.plain_random(seed, T)
    x[T // 2, col] = np.inf
    return x


def first_row(values, seed=61, T=16):
    """the first step's candidates ARE the first row's values (the root holds gap probability 1): plain rows behind it"""
    x = RC.plain_random(seed, T)
    x[0] = np.asarray(values, np.float32)
    return x


def at_low_edge():      # 2^-76 and its upper neighbour (one ulp apart: the smallest gap of the domain, scaled to exactly 2)
    return first_row([0.5, P_LO, np.nextafter(P_LO, np.float32(1)), 0.25, 0.125])


def below_low_edge():   # ... and its lower neighbour: one ulp outside
    return first_row([0.5, P_LO, np.nextafter(P_LO, np.float32(0)), 0.25, 0.125])


def at_high_edge():
    return first_row([0.5, P_HI, np.nextafter(P_HI, np.float32(0)), 0.25, 0.125])


def above_high_edge():
    return first_row([0.5, P_HI, np.nextafter(P_HI, np.float32(np.inf)), 0.25, 0.125])


def negative_column(seed, T=24):
    """column 3 negated, threshold -1: negative candidates (their words are below every non-negative one's)"""
    x = RC.plain_random(seed, T)
    x[:, 3] *= np.float32(-1.0)
    return x


def plus_zero(seed, T=T):
    """columns 3 and 4 are +0.0 under threshold 0: candidates of probability exactly 0 next to ordinary ones"""
    x = RC.plain_random(seed, T)
    x[:, 3:] = 0.0
    return x


# (name, threshold, reads): no step of any read holds a candidate outside the domain
def inside_launches():
    return [
        ("plain random", 0.05, np.stack([RC.plain_random(s) for s in (21, 22, 23, 24, 25)])),
        ("plain random thr 0", 0.0, np.stack([RC.plain_random(s, 24) for s in (26, 27)])),
        ("quantised", 0.0, np.stack([RC.quantised(s) for s in (1, 2, 3)])),
        ("two equal columns", 0.05, np.stack([RC.two_equal(s) for s in (1, 2)])),
        ("constant", 0.0, np.stack([RC.constant(), np.float32(0.5) * RC.constant()])),
        ("exact +0 among in-domain", 0.0, np.stack([plus_zero(s) for s in (41, 42, 43)])),
        ("zeros of both signs", 0.0, np.stack([RC.zero_cols(s) for s in (1, 2, 3, 4)])),  # (-0.0 ranks as +0: make_key)
    ]


# (name, threshold, reads, first): every read meets the guard; `first`: already on its first step
def outside_launches():
    return [
        ("scaled 2^-80", 0.0, np.stack([scaled(s, -80) for s in (1, 2, 3, 4)]), True),
        ("subnormal", 0.0, np.stack([RC.subnormal(s) for s in (1, 2)]), True),
        ("one column 2^-80", 0.0, np.stack([one_column(s, -80) for s in (5, 6, 7)]), True),
        ("scaled 2^30", 0.0, np.stack([scaled(s, 30) for s in (8, 9)]), False),  # (a small entry times 2^30 is still inside)
        ("one column 2^30", 0.0, np.stack([one_column(s, 30) for s in (10, 11, 12)]), False),
        ("one column 2^40", 0.0, np.stack([one_column(s, 40) for s in (13, 14)]), True),
        ("+inf", 0.0, np.stack([with_inf(51, 2), with_inf(52, 0)]), False),
        ("negative posteriors", -1.0, np.stack([negative_column(s) for s in (15, 16, 17)]), True),
        ("one ulp below 2^-76", 0.0, np.stack([below_low_edge(), below_low_edge()]), True),
        ("one ulp above 2^27", 0.0, np.stack([above_high_edge(), above_high_edge()]), True),
    ]


# (name, threshold, reads): the FIRST step is inside the domain with a candidate on its very edge (later steps may leave it:
# the edge candidate's descendants shrink or grow further)
def edge_launches():
    return [
        ("at 2^-76", 0.0, np.stack([at_low_edge(), at_low_edge()])),
        ("at 2^27", 0.0, np.stack([at_high_edge(), at_high_edge()])),
    ]


# (name, threshold, reads, (first half outside, second half outside)): two reads of one wavefront
def half_launches():
    a, b = RC.plain_random(71), scaled(72, -80)
    return [
        ("first half outside", 0.0, np.stack([b, a]), (True, False)),
        ("second half outside", 0.0, np.stack([a, b]), (False, True)),
        ("second half huge", 0.0, np.stack([a, scaled(73, 30)]), (False, True)),
    ]


def small_alphabet_launches():
    """(name, threshold, reads) for N = 3 and 4, the other members of the headline family: inside, tied, outside"""
    out = []
    for n in (3, 4):
        out.append(("N=%d plain" % n, 0.05, np.stack([scaled(80 + s, 0, n=n) for s in range(3)])))
        out.append(("N=%d quantised" % n, 0.0, np.stack([RC.quantised(s)[:, :n] for s in (1, 2)])))
        out.append(("N=%d scaled 2^-80" % n, 0.0, np.stack([scaled(90 + s, -80, n=n) for s in range(2)])))
        out.append(("N=%d scaled 2^30, plain" % n, 0.0, np.stack([scaled(95, 30, n=n), scaled(96, 0, n=n)])))
    return out


def crf_launches(S=4, T=32):
    """(name, reads, init): the CRF twin with 4 states -- inside, tiny, huge, zeros of both signs"""
    rng = np.random.default_rng(97)
    x = rng.random((4, T, S, N), dtype=np.float32)
    x /= x.sum(-1, keepdims=True)
    x = np.ascontiguousarray(x.astype(np.float32))
    init = np.ascontiguousarray(np.tile(np.array([0.1, 0.6, 0.2, 0.1], np.float32), (4, 1)))
    z = x.copy()
    z[:, :, :, 3:] = 0.0
    z[1, :, :, 3] = -0.0
    z[2, ::2, :, 2] *= -1.0
    return [
        ("crf inside", x, init),
        ("crf 2^-80", np.ascontiguousarray(x * np.float32(2.0 ** -80)), init),
        ("crf 2^30 and plain", np.ascontiguousarray(np.concatenate([x[:2] * np.float32(2.0 ** 30), x[2:]])), init),
        ("crf zeros and negatives", np.ascontiguousarray(z), init),
    ]


def run_all(fcd, beam):
    """every launch of this file against the oracle (the caller sets the tie order)"""
    for name, thr, x in inside_launches() + edge_launches():
        RC.check_plain(fcd, x, beam, thr, what=name)
    for name, thr, x, _ in outside_launches() + half_launches():
        RC.check_plain(fcd, x, beam, thr, what=name)
    for name, thr, x, _ in RC.failing_launches():
        RC.check_plain(fcd, x, beam, thr, what=name)
