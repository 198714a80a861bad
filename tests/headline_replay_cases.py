"""TEST INFRASTRUCTURE: constructed launches for the rare block of the headline beam kernels (two reads per wavefront, reads
of one length; csrc/beam_wave_step.inc, RSORT): a step whose kept candidates tie among more than 20 replays the
quicksort in registers, one flagged half after the other, with part of the step parked in LDS meanwhile.  Shared by
tests/test_headline_replay_emu.py (CPU, emulated kernels) and tests/test_gpu_headline_replay.py.

Beam 5, N = 5, T <= 64, at most 8 reads per launch; every read is compared with the oracle exactly (status, out_len, labels,
path) under both tie orders.  The smallest shapes on which the block can go wrong:
  all-equal rows (three steps in four from the third on have more than 20 candidates with the kept ones equal); a tie in only one half of the
  wavefront, either one; in both halves in the same step; an odd read count (the last wavefront's second half has no
  read); a tie in the step in which the other half's read fails (an empty candidate list, a NaN among several) or is left
  with a lone NaN; a tie in the step in which a node re-enters the beam (the branch serves both causes); a tie in the
  first row (five equal candidates: the recount) and in the last one (the quicksort); the CRF twin with 4 states.
profile() follows the reference's search (tests/naive_reference.py); the CPU test asserts from it and from the oracle's tie
counters that a case meets what it is named after."""
import numpy as np

import naive_reference as NV
import rank32_cases as RC

N = 5
T = 40
BEAM = 5
T0 = 9  # a step in which the all-equal read is flagged (asserted in the CPU test)


def failing_row(t0, T=T):
    """all-equal rows; row t0 lies below the threshold 0.05: the candidate list is empty (RanOutOfBeam)"""
    x = RC.constant(T)
    x[t0] = 0.01
    return x


def nan_row(t0, T=T):
    """all-equal rows; one NaN among the candidates of row t0 (IncomparableValues)"""
    x = RC.constant(T)
    x[t0, 3] = np.nan
    return x


def lone_nan_read(t0, T=T):
    """only column 1 passes the threshold 0.15; from row t0 on the read's one candidate is a NaN: never compared"""
    x = np.full((T, N), 0.1, np.float32)
    x[:, 1] = 0.7
    x[t0, 1] = np.nan
    return x


REENTRY_SEED = 11  # (a seed whose read meets a re-entering node in steps the all-equal read is flagged in; asserted in the CPU test)


def reentering(seed=REENTRY_SEED, T=64):
    return RC.plain_random(seed, T)


def profile(x, beam, thr):
    """per step of the reference's search: (the new beam's nodes, nodes of it that were in an EARLIER beam but not in the
    previous one -- they re-enter --, candidate count).  Stops at the step that fails."""
    thr = NV.f32(thr)
    rows = [[float(v) for v in r] for r in np.asarray(x, np.float32)]
    tree = NV.SuffixTree(N - 1)
    cur = [NV.Point1(NV.ROOT_NODE, 0, 0.0, 1.0)]
    seen, out = {NV.ROOT_NODE}, []
    for idx, pr in enumerate(rows):
        nxt = []
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
        try:
            srt = NV.sort_by_probability_desc(merged, NV.Point1.probability)
        except NV.SearchError:
            break
        if not srt:
            break
        prev = {c.node for c in cur}
        cur = srt[:beam]
        now = {c.node for c in cur}
        out.append((now, {n for n in now if n in seen and n not in prev}, len(srt)))
        seen |= now
        top = cur[0].probability()
        for c in cur:
            c.label_prob = NV.f32_div(c.label_prob, top)
            c.gap_prob = NV.f32_div(c.gap_prob, top)
    return out


def many_tie_steps(x, thr):
    """steps whose kept candidates tie among more than 20: the quicksort's"""
    return [t for t, s in enumerate(RC.tie_profile(x, BEAM, thr)) if "many" in s]


# (name, threshold, reads, expected statuses or None = all 0)
def launches():
    c, r = RC.constant(T), RC.plain_random(12, T)
    t0 = T0
    return [
        ("all equal", 0.0, np.stack([c, c]), None),
        ("first half only", 0.0, np.stack([c, r]), None),
        ("second half only", 0.0, np.stack([r, c]), None),
        ("both halves, different reads", 0.0, np.stack([c, np.float32(0.5) * c, RC.quantised(1, T), c]), None),
        ("odd read count", 0.0, np.stack([c, r, c]), None),
        ("the other half runs out of beam", 0.05, np.stack([c, failing_row(t0), failing_row(t0), c]), (0, 1, 1, 0)),
        ("the other half meets a NaN", 0.0, np.stack([c, nan_row(t0), nan_row(t0), c, nan_row(T - 1)]), (0, 2, 2, 0, 2)),
        ("the other half holds a lone NaN", 0.15, np.stack([c, lone_nan_read(t0), lone_nan_read(3), c]), None),
        ("a node re-enters", 0.0, np.stack([RC.constant(64), reentering(), reentering(), RC.constant(64)]), None),
        ("eight reads", 0.0, np.stack([c, r, RC.quantised(2, T), c, r, c, RC.two_equal(1, T), c]), None),
    ]


def crf_launch(T=T, S=4):
    """the CRF twin of the all-equal rows, and a quantised read in the other half"""
    x = np.full((3, T, S, N), 0.25, np.float32)
    x[1] = (np.random.default_rng(5).integers(1, 4, size=(T, S, N)) / 4.0).astype(np.float32)
    init = np.full((3, S), 0.25, np.float32)
    return np.ascontiguousarray(x), init


def counted_crf(x, init, thr=0.0):
    import session_cases as SC
    return SC.want_crf(x, init, BEAM, thr)[3]
