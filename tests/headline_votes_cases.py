"""TEST INFRASTRUCTURE: constructed inputs for the wave-wide votes of the headline beam kernels (csrc/beam_wave_step.inc, the
HL family: two reads per wavefront, reads of one length, N = 3, 4, 5 and the CRF twin with 4 states).  Their step forms
its lane predicates as masks -- a vote on every bare compare, joined in scalar registers -- and reads lane flags back from
them: the candidates of the step (m_valid), the nodes it creates (m_new), the kept candidates, the clash of equal
probabilities in the survivor table, the rank-domain guard, the fate of every child entry and the eviction store.
Shared by tests/test_headline_votes_emu.py (CPU, emulated kernels) and tests/test_gpu_headline_votes.py.

Every read is compared with the oracle: status, out_len, labels, path -- under both tie orders, beams 5 and 3.  Launches
of 1 .. 8 reads, T <= 48, the smallest at which each vote can go wrong:
  halves that differ (the per-half words of m_new, m_valid and alive_m): a launch of one read and of three (the last
    wavefront's second half has no read); a wavefront whose first half fails on its second step -- a NaN among several
    candidates, an empty candidate list -- while the second runs on, and the reverse;
  numbering: a step in which no lane creates a node (only the blank passes), a step in which every child lane of a full
    beam does (20 new nodes), the first step (the root alone);
  clash and guard: the INSIDE / OUTSIDE / HALVES tables of tests/rank_domain_cases.py on the CRF twin and on N = 3, 4; reads
    whose guarded step is also a step with a kept tie, so that both votes rise together;
  child fate: reads in which a child entry follows its node to a new slot, a child enters the beam for the first time, a
    node is evicted with a live ancestor (its row must be stored), the same node re-enters (its row is read back) and an
    evicted node is dead by the depth test.
step_profile() follows the reference's search (tests/naive_reference.py) and says, per step, which of these happen: the
CPU test asserts from it that the crafted reads reach the states they are named after."""
import numpy as np

import naive_reference as NV
import rank32_cases as RC
import rank_domain_cases as DC

N = RC.N
BEAMS = RC.BEAMS
INIT4 = np.array([0.1, 0.6, 0.2, 0.1], np.float32)


def step_profile(x, beam, thr, collapse=True):
    """per step of the reference's search, a dict:
      n_cand       merged candidates
      n_new        nodes created (tree.add_node calls)
      followed     children that were beam entries next to their parent and stay in the beam at ANOTHER slot
      entered      kept candidates that are extensions and have never been in the beam
      reentered    kept candidates that are extensions and have been in the beam before
      evicted_live beam entries that leave while a strictly shallower node stays (their child row is stored)
      evicted_dead beam entries that leave when every new beam entry is at least as deep (never stored)
    Stops at the step that fails."""
    x = np.asarray(x, np.float32)
    n = x.shape[1]
    thr = NV.f32(thr)
    rows = [[float(v) for v in r] for r in x]
    tree = NV.SuffixTree(n - 1)
    depth = {NV.ROOT_NODE: 0}
    cur = [NV.Point1(NV.ROOT_NODE, 0, 0.0, 1.0)]
    ever = {NV.ROOT_NODE}
    steps = []
    for idx, pr in enumerate(rows):
        old = {b.node: s for s, b in enumerate(cur)}
        before = len(tree.nodes)
        pairs = []  # (parent, child) for children that existed before this step and are beam entries
        nxt = []
        for b in cur:
            tip = tree.label(b.node)
            for label in range(n - 1):
                c = tree.get_child(b.node, label)
                if c is not None and c < before and c in old:
                    pairs.append((b.node, c))
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
                        depth[nn] = depth[b.node] + 1
                    if nn is not None:
                        nxt.append(NV.Point1(nn, 0, NV.f32(b.gap_prob * pb), 0.0))
                else:
                    nn = tree.get_child(b.node, label)
                    if nn is None:
                        nn = tree.add_node(b.node, label, idx)
                        depth[nn] = depth[b.node] + 1
                    nxt.append(NV.Point1(nn, 0, NV.f32(NV.f32(b.label_prob + b.gap_prob) * pb), 0.0))
        merged = []
        for item in NV.stable_sort_by_node(nxt):
            if merged and merged[-1].node == item.node:
                merged[-1].label_prob = NV.f32(merged[-1].label_prob + item.label_prob)
                merged[-1].gap_prob = NV.f32(merged[-1].gap_prob + item.gap_prob)
            else:
                merged.append(item)
        here = dict(n_cand=len(merged), n_new=len(tree.nodes) - before, followed=0, entered=0, reentered=0,
                    evicted_live=0, evicted_dead=0)
        try:
            srt = NV.sort_by_probability_desc(merged, NV.Point1.probability)
        except NV.SearchError:
            steps.append(here)
            break
        if not srt:
            steps.append(here)
            break
        cur = srt[:beam]
        new = {b.node: s for s, b in enumerate(cur)}
        dmin = min(depth[b.node] for b in cur)
        for parent, c in pairs:
            if c in new and new[c] != old[c]:
                here["followed"] += 1
        for node in new:
            if node not in old:
                here["reentered" if node in ever else "entered"] += 1
        for node in old:
            if node not in new:
                here["evicted_live" if depth[node] > dmin else "evicted_dead"] += 1
        ever |= set(new)
        steps.append(here)
        top = cur[0].probability()
        for c in cur:
            c.label_prob = NV.f32_div(c.label_prob, top)
            c.gap_prob = NV.f32_div(c.gap_prob, top)
    return steps


def met(x, beam, thr):
    """the events of step_profile() a read meets at all"""
    out = set()
    for s in step_profile(x, beam, thr):
        out |= {k for k in ("followed", "entered", "reentered", "evicted_live", "evicted_dead") if s[k]}
    return out


# ---- reads ----------------------------------------------------------------------------------------------------------
def fails_on_second_step(kind, seed, T=24):
    """plain rows; the SECOND step ends the read: a NaN among several candidates (threshold 0.05: the NaN passes, `pb < thr`
    is false) or a row nothing passes"""
    x = RC.plain_random(seed, T)
    if kind == "nan":
        x[1, 3] = np.nan
    else:
        x[1] = 0.01
    return x


def blank_only_rows(seed, T=24, first=8, n_rows=6):
    """plain rows, then `n_rows` rows only the blank passes (threshold 0.05): the tree is built, nobody creates a node"""
    x = RC.plain_random(seed, T)
    x[first:first + n_rows, 0] = 0.96
    x[first:first + n_rows, 1:] = 0.01
    return x


def twenty_new(T=16):
    """threshold 0.05.  Two label-only rows bring five fresh nodes of depth 2 into the beam, a blank-only row gives each of
    them a gap probability, and the fourth row lets every label of every one of them pass: 5 x 4 children, all new (a
    repeat creates its node because the gap probability is positive).  Plain rows behind it."""
    x = RC.plain_random(77, T)
    x[0] = [0.01, 0.40, 0.30, 0.19, 0.10]
    x[1] = [0.01, 0.11, 0.17, 0.29, 0.42]
    x[2] = [0.96, 0.01, 0.01, 0.01, 0.01]
    x[3] = [0.06, 0.31, 0.27, 0.21, 0.15]
    return x


def guarded_and_tied(seed, T=24):
    """quantised rows (equal products everywhere) scaled by 2^-80: a step outside the rank domain that holds a kept tie"""
    return (RC.quantised(seed, T) * np.float32(2.0 ** -80)).astype(np.float32)


def both_votes_steps(x, beam, thr):
    """steps that are outside the rank domain AND hold a kept tie"""
    out = DC.outside_steps(x, beam, thr)
    tie = RC.tie_profile(x, beam, thr)
    return sum(1 for o, t in zip(out, tie) if o and (t & {"top", "inside", "boundary"}))


FATE_SEEDS = (102, 105, 106, 107)  # (the first three meet all five events under both beams: asserted in the CPU test)


# ---- launches: (name, threshold, reads) -----------------------------------------------------------------------------
def halves_launches():
    a, b = RC.plain_random(81, 24), RC.plain_random(82, 24)
    return [
        ("one read", 0.05, np.stack([RC.plain_random(83)])),
        ("three reads", 0.05, np.stack([RC.plain_random(s) for s in (84, 85, 86)])),
        ("first half: NaN among several", 0.05, np.stack([fails_on_second_step("nan", 87), a])),
        ("second half: NaN among several", 0.05, np.stack([a, fails_on_second_step("nan", 87)])),
        ("first half: empty list", 0.05, np.stack([fails_on_second_step("empty", 88), b])),
        ("second half: empty list", 0.05, np.stack([b, fails_on_second_step("empty", 88)])),
    ]


def numbering_launches():
    return [
        ("no new node", 0.05, np.stack([blank_only_rows(91), blank_only_rows(92, first=5), RC.plain_random(93, 24)])),
        ("twenty new nodes", 0.05, np.stack([twenty_new(), RC.plain_random(94, 16)])),
    ]


def both_votes_launches():
    return [("guarded and tied", 0.0, np.stack([guarded_and_tied(s) for s in (1, 2, 3)]))]


def fate_launches():
    return [("child fate", 0.05, np.stack([RC.plain_random(s) for s in FATE_SEEDS]))]


def plain_launches():
    return halves_launches() + numbering_launches() + both_votes_launches() + fate_launches()


def domain_tables():
    """(name, threshold, reads) of rank_domain_cases: INSIDE (with the edges), OUTSIDE, HALVES"""
    return ([(n, t, x) for n, t, x in DC.inside_launches() + DC.edge_launches()]
            + [(n, t, x) for n, t, x, _ in DC.outside_launches() + DC.half_launches()])


def as_crf(x, S=4):
    """a launch of plain reads (B, T, N) as one of the CRF search with S states that all see the same row"""
    x = np.asarray(x, np.float32)
    return (np.ascontiguousarray(np.repeat(x[:, :, None, :], S, axis=2)),
            np.ascontiguousarray(np.tile(INIT4[:S], (x.shape[0], 1))))


def small_alphabet(x, n):
    """the first n columns of a launch: the N = 3 and N = 4 members of the family"""
    return np.ascontiguousarray(np.asarray(x, np.float32)[:, :, :n])


def run_plain(fcd, beam):
    """N = 5: this file's own launches (the caller sets the tie order)"""
    for name, thr, x in plain_launches():
        RC.check_plain(fcd, x, beam, thr, what=name)


def run_small(fcd, beam, n):
    """N = 3 or 4: this file's launches and the domain tables, cut to n columns"""
    for name, thr, x in plain_launches() + domain_tables():
        RC.check_plain(fcd, small_alphabet(x, n), beam, thr, what="N=%d %s" % (n, name))


def run_crf(fcd, beam):
    """the CRF twin with 4 states: this file's launches and the domain tables"""
    for name, thr, x in plain_launches() + domain_tables():
        x4, init = as_crf(x)
        RC.check_crf(fcd, x4, init, beam, thr, what="crf " + name)
