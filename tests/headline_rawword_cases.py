"""TEST INFRASTRUCTURE: constructed launches for the raw probability table of the headline beam kernels (two reads per
wavefront, reads of one length; csrc/beam_wave_step.inc, RAWK): the every-step path writes bits(prob + 0.0f) alone and ranks
on it; the keyed probability word and the node word exist only inside the step's rare block, which rebuilds both tables
before the recount, the quicksort replay and the second settling read them.  Shared by tests/test_headline_rawword_emu.py
(CPU, emulated kernels) and tests/test_gpu_headline_rawword.py.

Beam 5, N = 5, reads of 1 to 130 rows, at most 8 reads per launch; every read is compared with the oracle exactly (status,
out_len, labels, path) under both tie orders, as plain reads (S = 0) and as the CRF twin with 4 states.
  kept ties decided by the node word: rows of powers of two (every product of the search is exact, so equal probabilities are
    bit-equal) -- a slot's own candidate against a new child, two new children of one step, an existing child entry against a
    slot's own candidate; each once inside the beam and once across its boundary (TIE_SEEDS, found by search, asserted);
  more than 20 candidates with a kept tie (the quicksort replay behind the rebuild): in the lower half only, the upper half
    only, both halves in one step, and in consecutive steps (all-equal rows: each such step overwrites the keyed tables with
    raw words at its top and rebuilds them);
  guarded steps (the recount serves them too): one candidate below 2^-76, negative ones (the only words on which raw and keyed
    order differ), a NaN, a +inf, and candidates of probability 0 beside empty slots (both hold word 0);
  a step that takes the rare branch for a returning node only: nothing is rebuilt, and the tables are not read.
report() follows the reference's search (tests/naive_reference.py); the CPU test asserts from it, and from the oracle's tie
counters, that every case reaches what it is named after."""
import numpy as np

import naive_reference as NV
import rank32_cases as RC
import rank_domain_cases as DC

N = 5
BEAM = 5
KINDS = ("self", "new", "child")  # a slot's own candidate / a node created in this step / a child entry that existed


def report(x, beam=BEAM, thr=0.0):
    """per step of the reference's search, a dict: n (candidates), ties (set of (kinds of the two neighbours, where) for equal
    neighbours of the sorted list with the first one kept: where = "inside" | "boundary"), many (a kept tie among more than
    20), outside (a candidate outside the f32 count's domain), negative (two or more negative candidates), zero (a candidate
    of probability 0), back (a node that was in an earlier beam, not in the previous one, is kept).  Stops at a failing step."""
    thr = NV.f32(thr)
    rows = [[float(v) for v in r] for r in np.asarray(x, np.float32)]
    tree = NV.SuffixTree(N - 1)
    cur = [NV.Point1(NV.ROOT_NODE, 0, 0.0, 1.0)]
    seen, steps = {NV.ROOT_NODE}, []
    for idx, pr in enumerate(rows):
        nxt, fresh = [], set()

        def child_of(b, label):
            nn = tree.get_child(b.node, label)
            if nn is None:
                nn = tree.add_node(b.node, label, idx)
                fresh.add(nn)
            return nn

        for b in cur:
            tip = tree.label(b.node)
            if pr[0] > thr:
                nxt.append(NV.Point1(b.node, 0, 0.0, NV.f32(NV.f32(b.label_prob + b.gap_prob) * pr[0])))
            for label in range(N - 1):
                pb = pr[label + 1]
                if pb < thr:
                    continue
                if label == tip:
                    nxt.append(NV.Point1(b.node, 0, NV.f32(b.label_prob * pb), 0.0))
                    if tree.get_child(b.node, label) is not None or b.gap_prob > 0.0:
                        nxt.append(NV.Point1(child_of(b, label), 0, NV.f32(b.gap_prob * pb), 0.0))
                else:
                    nxt.append(NV.Point1(child_of(b, label), 0, NV.f32(NV.f32(b.label_prob + b.gap_prob) * pb), 0.0))
        merged = []
        for item in NV.stable_sort_by_node(nxt):
            if merged and merged[-1].node == item.node:
                merged[-1].label_prob = NV.f32(merged[-1].label_prob + item.label_prob)
                merged[-1].gap_prob = NV.f32(merged[-1].gap_prob + item.gap_prob)
            else:
                merged.append(item)
        probs = [c.probability() for c in merged]
        st = {"n": len(merged), "outside": any(not DC.in_domain(p) for p in probs),
              "negative": sum(1 for p in probs if p < 0.0) >= 2, "zero": any(p == 0.0 for p in probs),
              "ties": set(), "many": False, "back": False}
        try:
            srt = NV.sort_by_probability_desc(merged, NV.Point1.probability)
        except NV.SearchError:
            steps.append(st)
            break
        if not srt:
            steps.append(st)
            break
        prev = {c.node for c in cur}
        kind = lambda c: "self" if c.node in prev else ("new" if c.node in fresh else "child")
        p = [c.probability() for c in srt]
        for j in range(min(beam, len(p) - 1)):
            if p[j] == p[j + 1]:
                st["ties"].add((tuple(sorted((kind(srt[j]), kind(srt[j + 1])))), "inside" if j + 1 < beam else "boundary"))
                st["many"] = st["many"] or len(p) > 20
        cur = srt[:beam]
        st["back"] = any(c.node in seen and c.node not in prev for c in cur)
        seen |= {c.node for c in cur}
        steps.append(st)
        top = cur[0].probability()
        for c in cur:
            c.label_prob = NV.f32_div(c.label_prob, top)
            c.gap_prob = NV.f32_div(c.gap_prob, top)
    return steps


def ties_met(x, thr=0.0):
    out = set()
    for s in report(x, BEAM, thr):
        out |= s["ties"]
    return out


def many_steps(x, thr=0.0):
    return [t for t, s in enumerate(report(x, BEAM, thr)) if s["many"]]


# ---- reads ----------------------------------------------------------------------------------------------------------
def dyadic(seed, T, lo=-3):
    """rows of powers of two, 2^lo .. 2^-1: every product of the search is exact"""
    return np.ldexp(np.float32(1.0), np.random.default_rng(seed).integers(lo, 0, size=(T, N))).astype(np.float32)


# the six (pair of candidate kinds, where the tie sits) classes, each with a (seed, rows) whose dyadic read meets it
PAIRS = (("new", "self"), ("new", "new"), ("child", "self"))
TIE_SEEDS = {
    (("new", "self"), "inside"): (0, 24), (("new", "self"), "boundary"): (2, 24),
    (("new", "new"), "inside"): (1, 24), (("new", "new"), "boundary"): (3, 24),
    (("child", "self"), "inside"): (6, 24), (("child", "self"), "boundary"): (10, 24),
}


def tie_read(pair, where):
    seed, T = TIE_SEEDS[(pair, where)]
    return dyadic(seed, T)


BACK_SEED = 11  # plain random rows, no two candidates ever equal, nothing outside the domain: a node re-enters (asserted)


def back_read(T=64):
    return RC.plain_random(BACK_SEED, T)


def back_only_steps(x, thr=0.0):
    """steps that take the rare branch for a returning node alone: no kept tie, no candidate outside the domain"""
    return [t for t, s in enumerate(report(x, BEAM, thr)) if s["back"] and not s["ties"] and not s["outside"]]


def zero_beside_empty(seed, T=24):
    """columns 3 and 4 are +0.0 under threshold 0 from the FIRST row on, where the root's five candidates leave twenty slots
    empty: candidates of probability 0 and empty slots, both word 0"""
    return DC.plus_zero(seed, T)


def nan_among(T=12):
    return RC.nan_among(T)


# (name, threshold, reads, expected statuses or None = all 0)
def launches():
    c, r = RC.constant(40), RC.plain_random(12, 40)
    ties = [tie_read(p, w) for p in PAIRS for w in ("inside", "boundary")]
    Tt = max(t.shape[0] for t in ties)
    assert all(t.shape[0] == Tt for t in ties)
    return [
        ("kept ties decided by the node word", 0.0, np.stack(ties), None),
        ("one row", 0.0, np.stack([dyadic(1, 1), dyadic(2, 1), RC.constant(1)]), None),
        ("130 rows", 0.0, np.stack([dyadic(3, 130), RC.constant(130)]), None),
        ("many, lower half only", 0.0, np.stack([c, r]), None),
        ("many, upper half only", 0.0, np.stack([r, c]), None),
        ("many, both halves", 0.0, np.stack([c, np.float32(0.5) * c, c]), None),
        ("below 2^-76", 0.0, np.stack([DC.one_column(5, -80, T=24), RC.plain_random(21, 24)]), None),
        ("negative", -1.0, np.stack([DC.negative_column(15), DC.negative_column(16), RC.plain_random(22, 24)]), None),
        ("a NaN", 0.0, np.stack([nan_among(), RC.plain_random(33, 12), dyadic(4, 12)]), (2, 0, 0)),
        # (the step that holds the +inf ranks it, guarded; the next one divides inf by inf and fails on the NaN)
        ("+inf", 0.0, np.stack([DC.with_inf(51, 2), DC.with_inf(52, 0)]), (2, 2)),
        ("zero beside empty slots", 0.0, np.stack([zero_beside_empty(41), zero_beside_empty(42)]), None),
        ("a returning node only", 0.0, np.stack([back_read(), back_read()]), None),
    ]


def crf_launches(S=4, T=40):
    """(name, reads, init) for the CRF twin with 4 states: dyadic rows (kept ties), all-equal rows (more than 20 candidates
    tied, step after step), negative columns and zeros"""
    rng = np.random.default_rng(7)
    d = np.ldexp(np.float32(1.0), rng.integers(-3, 0, size=(3, T, S, N))).astype(np.float32)
    init = np.ascontiguousarray(np.tile(np.array([0.125, 0.5, 0.25, 0.125], np.float32), (3, 1)))
    e = np.full((3, T, S, N), 0.25, np.float32)
    e[1] = d[1]
    z = rng.random((3, T, S, N), dtype=np.float32)
    z[0, :, :, 3] *= np.float32(-1.0)
    z[1, :, :, 3:] = 0.0
    z[2, :, :, 2] *= np.float32(2.0 ** -80)
    return [("crf dyadic", np.ascontiguousarray(d), init), ("crf all equal", np.ascontiguousarray(e), init),
            ("crf negative, zero, tiny", np.ascontiguousarray(z), init)]


def run_plain(fcd):
    for name, thr, x, _ in launches():
        RC.check_plain(fcd, x, BEAM, thr, what=name)


def run_crf(fcd):
    for name, x, init in crf_launches():
        RC.check_crf(fcd, x, init, BEAM, -1.0 if "negative" in name else 0.0, what=name)
