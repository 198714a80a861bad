"""TEST INFRASTRUCTURE: constructed launches for the wave-uniform predicates of the headline beam kernels (two reads per
wavefront, reads of one length; csrc/beam_wave_step.inc, HL).  Adopted: "this group's own candidate was dropped", the
eviction store's mask, is a multiple of the kept own-lane bits in scalar registers instead of an LDS look-up, and the new
nodes' ids are counted with a lane-constant word.  Priced and not adopted ("Wave-uniform predicates"):
a half's candidate count, beam width and group mask in scalar registers, eviction stores without the dead-row test -- the cases
written for them (widths that differ between the halves, a half that runs out, the numbering of the upper half, a recount
behind a width change) stay: they are the states in which those forms go wrong, whoever tries them next.
Shared by tests/test_headline_scalar_emu.py (CPU, emulated kernels) and tests/test_gpu_headline_scalar.py.

Beam 5, N = 5, two to four reads of one length per launch (one or two wavefronts), at most 130 rows; every read is compared
with the oracle exactly (status, out_len, labels, path) under both tie orders, as plain reads (S = 0) and as the CRF twin
with 4 states (every state carries the same rows, so the twin's search is the trace's with collapse off and an init row).

trace() follows the reference's search (tests/naive_reference.py) and records per step what the kernel's masks hold; the
CPU test asserts from it that every case reaches the state it is named after:
  widths        the two halves of a wavefront hold different beam widths in the same step, every width 1 .. 5 occurs, and a
                read's width shrinks and later grows again while its neighbour is full;
  runs out      a half has no candidate while the other runs on (status 1, out_len 0), in the middle and in the last step;
  NaN           a NaN among two or more candidates fails the read (status 2); a lone NaN does not;
  eviction      a node is evicted and later re-enters the beam (the reload reads its stored row: the emulator aborts on a
                row that was never written), and an evicted node every new beam entry is at least as deep as -- the row the
                dead-row test skips.  (Such a node cannot return, that is the test's argument; a kernel that stores its
                row as well must disturb nothing.)
  patterns      steps in which all five slots keep their own candidate, none does, and only slot 4 does -- the end bits of
                the replication -- with the read in the lower half and in the upper half;
  new ids       both halves create more than 16 nodes in the same step: ids of the upper half that ran on from the lower
                half's would leave the step's block of 32;
  recount       a step with a kept tie or a candidate outside the count's domain directly behind a step that changed the
                width."""
import numpy as np

import naive_reference as NV
import rank32_cases as RC
import rank_domain_cases as DC

N = 5
BEAM = 5
S = 4
INIT = np.array([0.125, 0.5, 0.25, 0.125], np.float32)


def trace(x, thr=0.0, crf=False, beam=BEAM):
    """per step, a dict: n (merged candidates), before / width (beam entries in front of and behind the step), own (per slot
    of the beam in front of the step: its node is kept), new (nodes created), back (a kept node was in an earlier beam and not
    in the previous one), dead (an evicted node no deeper than every new beam entry), recount (a kept tie, or a candidate
    outside the f32 count's domain), fail ("empty" | "nan" | None), lone_nan.  Stops at a failing step.
    crf: x is the plain read every state of the twin carries; no collapse, the root holds INIT."""
    thr = NV.f32(thr)
    rows = [[float(v) for v in r] for r in np.asarray(x, np.float32)]
    tree = NV.SuffixTree(N - 1)
    cur = [NV.Point1(NV.ROOT_NODE, 0, float(INIT.max()), float(INIT[0]))] if crf else [NV.Point1(NV.ROOT_NODE, 0, 0.0, 1.0)]
    depth = {NV.ROOT_NODE: 0}
    seen, steps = {NV.ROOT_NODE}, []
    for idx, pr in enumerate(rows):
        nxt, created = [], 0
        for b in cur:
            tip = tree.label(b.node)
            if pr[0] > thr:
                nxt.append(NV.Point1(b.node, 0, 0.0, NV.f32(NV.f32(b.label_prob + b.gap_prob) * pr[0])))
            for label in range(N - 1):
                pb = pr[label + 1]
                if pb < thr:
                    continue
                rep = (not crf) and label == tip
                if rep:
                    nxt.append(NV.Point1(b.node, 0, NV.f32(b.label_prob * pb), 0.0))
                nn = tree.get_child(b.node, label)
                if nn is None and (not rep or b.gap_prob > 0.0):
                    nn = tree.add_node(b.node, label, idx)
                    depth[nn] = depth[b.node] + 1
                    created += 1
                if nn is not None:
                    nxt.append(NV.Point1(nn, 0, NV.f32((b.gap_prob if rep else NV.f32(b.label_prob + b.gap_prob)) * pb), 0.0))
        merged = []
        for item in NV.stable_sort_by_node(nxt):
            if merged and merged[-1].node == item.node:
                merged[-1].label_prob = NV.f32(merged[-1].label_prob + item.label_prob)
                merged[-1].gap_prob = NV.f32(merged[-1].gap_prob + item.gap_prob)
            else:
                merged.append(item)
        probs = [c.probability() for c in merged]
        st = {"n": len(merged), "before": len(cur), "width": 0, "own": (), "new": created, "back": False, "dead": False,
              "recount": any(not DC.in_domain(p) for p in probs), "fail": None,
              "lone_nan": len(probs) == 1 and probs[0] != probs[0]}
        steps.append(st)
        if not merged:
            st["fail"] = "empty"
            break
        try:
            srt = NV.sort_by_probability_desc(merged, NV.Point1.probability)
        except NV.SearchError:
            st["fail"] = "nan"
            break
        p = [c.probability() for c in srt]
        st["recount"] = st["recount"] or any(p[j] == p[j + 1] for j in range(min(beam, len(p) - 1)))
        prev = [c.node for c in cur]
        cur = srt[:beam]
        kept = {c.node for c in cur}
        st["width"] = len(cur)
        st["own"] = tuple(nd in kept for nd in prev)
        st["back"] = any(c.node in seen and c.node not in prev for c in cur)
        shallow = min(depth[c.node] for c in cur)
        st["dead"] = any(nd not in kept and depth[nd] <= shallow for nd in prev)
        seen |= kept
        top = cur[0].probability()
        for c in cur:
            c.label_prob = NV.f32_div(c.label_prob, top)
            c.gap_prob = NV.f32_div(c.gap_prob, top)
    return steps


# ---- reads ----------------------------------------------------------------------------------------------------------
def peaky(seed, T, p_pass=0.3):
    """peaky rows: every column passes the threshold THR_PEAKY with probability p_pass (at least one does), with a value in
    [0.1, 0.9); the others hold 0.001.  A slot that sees no blank and whose extension is already a beam entry adds no
    candidate of its own (plain search: a node just created has gap probability 0 and no repeat child), so the candidate
    count falls below the beam width and rises again.  (The CRF search has no repeat-stay: every slot adds a candidate in
    every step that succeeds, so there the width only ever grows.)"""
    rng = np.random.default_rng(seed)
    on = rng.random((T, N)) < p_pass
    on[np.arange(T), rng.integers(0, N, size=T)] = True
    v = (0.1 + 0.8 * rng.random((T, N))).astype(np.float32)
    return np.where(on, v, np.float32(0.001)).astype(np.float32)


def empty_at(seed, T, at):
    """plain random rows; row `at` passes nothing under threshold 0.05"""
    x = RC.plain_random(seed, T)
    x[at] = 0.01
    return x


def nan_at(seed, T, at):
    x = RC.plain_random(seed, T)
    x[at, 3] = np.nan
    return x


def fanout(seed, T=12):
    """rows that pass the four labels alone (even rows) and the blank alone (odd rows) under THR_PEAKY: a label row keeps five
    fresh leaves, the blank row gives each a gap probability, and the next label row creates all twenty children"""
    rng = np.random.default_rng(seed)
    x = np.full((T, N), 0.001, np.float32)
    x[0::2, 1:] = (0.1 + 0.2 * rng.random((len(x[0::2]), N - 1))).astype(np.float32)
    x[1::2, 0] = np.float32(0.9)
    return x


# (seeds found by search over trace(), asserted in the CPU test)
WIDTH_SEEDS = (42, 1)       # peaky reads: 42 holds every width 1 .. 5 and shrinks 3 -> 2; 1 shrinks 5 -> 4 and 5 -> 3
WIDTH_T = 40
PATTERN_SEED = 389          # rank32_cases.plain_random: all five own candidates kept / none kept / only slot 4's kept
PATTERN_T = 64
BACK_SEEDS = (11, 15)       # rank32_cases.plain_random: a node re-enters (11: plain search; 15: plain and the CRF twin)
BACK_T = 64
RECOUNT_SEED = 31
RECOUNT_T = 48
THR_PEAKY = 0.02


def width_reads():
    return [peaky(s, WIDTH_T) for s in WIDTH_SEEDS]


def pattern_read():
    return RC.plain_random(PATTERN_SEED, PATTERN_T)


def recount_read():
    """quantised peaky rows: equal probabilities are bit-equal, and the threshold moves the width"""
    x = peaky(RECOUNT_SEED, RECOUNT_T)
    return (np.round(x * np.float32(64.0)) / np.float32(64.0)).astype(np.float32)


# (name, threshold, reads, expected statuses or None = all 0)
def launches():
    full = RC.plain_random(12, WIDTH_T)
    w0, w1 = width_reads()
    pat, fullp = pattern_read(), RC.plain_random(13, PATTERN_T)
    back, back2 = (RC.plain_random(s, BACK_T) for s in BACK_SEEDS)
    rec, fullr = recount_read(), RC.plain_random(14, RECOUNT_T)
    lone = RC.lone_nan(0x7FC00000)
    return [
        ("widths, narrow below full", THR_PEAKY, np.stack([w0, full]), None),
        ("widths, full below narrow", THR_PEAKY, np.stack([full, w1]), None),
        ("widths, two narrow halves, two wavefronts", THR_PEAKY, np.stack([w0, w1, w1, w0]), None),
        ("runs out, lower half", 0.05, np.stack([empty_at(35, 24, 12), RC.plain_random(36, 24)]), (1, 0)),
        ("runs out, upper half", 0.05, np.stack([RC.plain_random(36, 24), empty_at(35, 24, 12)]), (0, 1)),
        ("runs out in the last step", 0.05, np.stack([empty_at(35, 24, 23), RC.plain_random(36, 24), RC.plain_random(37, 24),
                                                      empty_at(38, 24, 23)]), (1, 0, 0, 1)),
        ("NaN among several", 0.0, np.stack([nan_at(31, 12, 6), RC.plain_random(33, 12), RC.plain_random(34, 12),
                                             nan_at(39, 12, 11)]), (2, 0, 0, 2)),
        ("lone NaN", 0.5, np.stack([lone, RC.lone_nan(0xFFFFFFFF)]), None),
        ("eviction and re-entry", 0.0, np.stack([back, back2, back2, back]), None),
        ("eviction patterns, lower half", 0.0, np.stack([pat, fullp]), None),
        ("eviction patterns, upper half", 0.0, np.stack([fullp, pat]), None),
        ("new ids in both halves", THR_PEAKY, np.stack([fanout(17), fanout(18)]), None),
        ("recount behind a width change, lower half", THR_PEAKY, np.stack([rec, fullr]), None),
        ("recount behind a width change, upper half", THR_PEAKY, np.stack([fullr, rec]), None),
    ]


def by_name():
    return {name: (thr, x, sts) for name, thr, x, sts in launches()}


def crf_twin(x):
    """[B, T, N] plain reads -> ([B, T, S, N], init): every state carries the read's rows"""
    xs = np.ascontiguousarray(np.repeat(np.asarray(x, np.float32)[:, :, None, :], S, axis=2))
    return xs, np.ascontiguousarray(np.tile(INIT, (x.shape[0], 1)))


def run_plain(fcd):
    for name, thr, x, _ in launches():
        RC.check_plain(fcd, x, BEAM, thr, what=name)


def run_crf(fcd):
    for name, thr, x, _ in launches():
        xs, init = crf_twin(x)
        RC.check_crf(fcd, xs, init, BEAM, thr, what=name)
