"""TEST INFRASTRUCTURE: constructed launches for three forms of the headline beam step (two reads per wavefront, reads of one
length; csrc/beam_wave_step.inc, HL):
  WSC   the beam width as loop-carried scalar state -- the group mask and the two halves' widths, formed afresh in the step's
        first rare block when a running half's capped candidate count differs from its width;
  ZSEL  no select where the value is already zero -- the pushed extension of a slot nobody pushed to, and the gap probability
        of a slot's own and its group's spare lane under one mask;
  CHB   the new slot's child entry gathered through bit 0 of the survivor-table entry, without a look at the source's kind.
Shared by tests/test_headline_width_emu.py (CPU, emulated kernels: there the step checks the carried state, the pushed word
and the gathered entry against the forms they replace, in every step, and aborts) and tests/test_gpu_headline_width.py.

N = 5, beams 1 .. 5, one to four reads of one length per launch, at most 130 rows; every read is compared with the oracle
exactly (status, out_len, labels, path) under both tie orders, as plain reads (S = 0) and as the CRF twin with 4 states
(tests/headline_scalar_cases.py: every state carries the same rows).

trace() follows the reference's search (tests/naive_reference.py); the CPU test asserts from it that every case reaches the
situation it is named after:
  widths     grow 1 -> 5 over the first steps; shrink and grow again mid-read under a threshold that cuts most of a row;
             differ between the halves and change in one half only; a half runs out while the other goes on; a NaN fails one
             half in the step in which the other's width changes; a launch of three reads and of one;
  pushes     an extension into a beam entry whose contribution is exactly 0 under threshold 0; a slot that is a candidate only
             through its incoming extension; a kept slot whose blank passed (its gap probability is what the spare lane
             divides); a -0.0 posterior under threshold 0;
  sources    new beam entries whose source is a slot's own candidate, a child entering the beam for the first time and a
             returning node, all in one step; a returning node one of whose children is a beam entry of the same step (its
             reloaded row points at a current slot)."""
import numpy as np

import headline_scalar_cases as HS
import naive_reference as NV
import rank32_cases as RC

N = 5
BEAMS = (1, 2, 3, 4, 5)
THR_PEAKY = HS.THR_PEAKY


def trace(x, thr=0.0, crf=False, beam=5):
    """per step, a dict: before / width (beam entries in front of and behind the step), n (merged candidates), fail ("empty" |
    "nan" | None), zero_push (an extension into a node of the beam in front of the step contributes exactly 0), inc_only (a
    node of the beam in front of the step is a candidate through an incoming extension alone: no blank, no repeat-stay),
    blank_kept (a kept candidate is its slot's own and its blank passed), kinds (of the new beam's entries: "self" the node
    was in the beam in front of the step, "first" it has never been in a beam, "back" it has, but not in the last one),
    back_child (a "back" entry has a child that is an entry of the same new beam).  Stops at a failing step.
    crf: x is the plain read every state of the twin carries; no collapse, the root holds HS.INIT."""
    thr = NV.f32(thr)
    rows = [[float(v) for v in r] for r in np.asarray(x, np.float32)]
    tree = NV.SuffixTree(N - 1)
    cur = [NV.Point1(NV.ROOT_NODE, 0, float(HS.INIT.max()), float(HS.INIT[0]))] if crf else [NV.Point1(NV.ROOT_NODE, 0, 0.0, 1.0)]
    seen, steps = {NV.ROOT_NODE}, []
    for idx, pr in enumerate(rows):
        prev = [c.node for c in cur]
        nxt, own_terms, incoming = [], {}, {}
        zero_push = False
        for b in cur:
            tip = tree.label(b.node)
            if pr[0] > thr:
                nxt.append(NV.Point1(b.node, 0, 0.0, NV.f32(NV.f32(b.label_prob + b.gap_prob) * pr[0])))
                own_terms.setdefault(b.node, set()).add("blank")
            for label in range(N - 1):
                pb = pr[label + 1]
                if pb < thr:
                    continue
                rep = (not crf) and label == tip
                if rep:
                    nxt.append(NV.Point1(b.node, 0, NV.f32(b.label_prob * pb), 0.0))
                    own_terms.setdefault(b.node, set()).add("stay")
                nn = tree.get_child(b.node, label)
                if nn is None and (not rep or b.gap_prob > 0.0):
                    nn = tree.add_node(b.node, label, idx)
                if nn is not None:
                    contrib = NV.f32((b.gap_prob if rep else NV.f32(b.label_prob + b.gap_prob)) * pb)
                    nxt.append(NV.Point1(nn, 0, contrib, 0.0))
                    if nn in prev:
                        incoming[nn] = True
                        zero_push = zero_push or contrib == 0.0
        merged = []
        for item in NV.stable_sort_by_node(nxt):
            if merged and merged[-1].node == item.node:
                merged[-1].label_prob = NV.f32(merged[-1].label_prob + item.label_prob)
                merged[-1].gap_prob = NV.f32(merged[-1].gap_prob + item.gap_prob)
            else:
                merged.append(item)
        st = {"n": len(merged), "before": len(cur), "width": 0, "fail": None, "zero_push": zero_push,
              "inc_only": any(nd not in own_terms for nd in incoming), "blank_kept": False, "kinds": set(), "back_child": False}
        steps.append(st)
        if not merged:
            st["fail"] = "empty"
            break
        try:
            srt = NV.sort_by_probability_desc(merged, NV.Point1.probability)
        except NV.SearchError:
            st["fail"] = "nan"
            break
        cur = srt[:beam]
        kept = {c.node for c in cur}
        st["width"] = len(cur)
        st["blank_kept"] = any(c.node in prev and "blank" in own_terms.get(c.node, ()) and c.gap_prob > 0.0 for c in cur)
        for c in cur:
            kind = "self" if c.node in prev else ("back" if c.node in seen else "first")
            st["kinds"].add(kind)
            if kind == "back" and any(tree.get_child(c.node, label) in kept for label in range(N - 1)):
                st["back_child"] = True
        seen |= kept
        top = cur[0].probability()
        for c in cur:
            c.label_prob = NV.f32_div(c.label_prob, top)
            c.gap_prob = NV.f32_div(c.gap_prob, top)
    return steps


def widths(tr):
    return [s["width"] for s in tr]


# ---- reads ----------------------------------------------------------------------------------------------------------
GROW_T = 16


def growing(label=1, T=GROW_T):
    """threshold THR_PEAKY.  The first row passes the blank alone (the root stays alone: width 1); every later row passes the
    blank and one label, so that each step adds the next repeat of that label to the beam: widths 1, 2, 3, 4, 5"""
    x = np.full((T, N), 0.001, np.float32)
    x[:, 0] = 0.6
    x[1:, label] = 0.3
    return x


def nan_beside(at, T):
    """plain rows with a NaN label in row `at`: several candidates, one of them a NaN -- the read fails there"""
    x = RC.plain_random(51, T)
    x[at, 3] = np.nan
    return x


ZERO_SEEDS = (1, 2)   # rank32_cases.zero_cols: zero and -0.0 posteriors under threshold 0
KIND_SEEDS = (11, 28)  # rank32_cases.plain_random: 11 meets both source cases as a plain read, 28 as the CRF twin (found by search over trace())
KIND_T = HS.BACK_T


def width_change_step(tr):
    """the first step behind the read's start-up in which the width changes"""
    return next(t for t in range(6, len(tr)) if tr[t]["width"] != tr[t]["before"])


# (name, threshold, reads, expected statuses or None = all 0); every launch runs under every beam of BEAMS
def launches():
    w0, w1 = HS.width_reads()
    full = RC.plain_random(12, HS.WIDTH_T)
    at = width_change_step(trace(w0, THR_PEAKY))
    by = HS.by_name()
    out = [
        ("widths grow", THR_PEAKY, np.stack([growing(1), growing(3)]), None),
        ("widths grow, one read", THR_PEAKY, np.stack([growing(2)]), None),
        ("widths shrink and grow, narrow below full", THR_PEAKY, np.stack([w0, full]), None),
        ("widths shrink and grow, full below narrow", THR_PEAKY, np.stack([full, w1]), None),
        ("widths, two narrow halves", THR_PEAKY, np.stack([w0, w1]), None),
        ("widths, three reads", THR_PEAKY, np.stack([w1, w0, w1]), None),
        ("runs out, lower half",) + by["runs out, lower half"],
        ("runs out, upper half",) + by["runs out, upper half"],
        ("NaN beside a width change, lower half", THR_PEAKY, np.stack([nan_beside(at, HS.WIDTH_T), w0]), (2, 0)),
        ("NaN beside a width change, upper half", THR_PEAKY, np.stack([w0, nan_beside(at, HS.WIDTH_T)]), (0, 2)),
        ("zero pushes", 0.0, np.stack([RC.zero_cols(s) for s in ZERO_SEEDS] + [RC.zero_cols(ZERO_SEEDS[0])]), None),
        ("source kinds", 0.0, np.stack([RC.plain_random(s, KIND_T) for s in KIND_SEEDS]), None),
        ("source kinds, peaky", THR_PEAKY, np.stack([HS.peaky(s, KIND_T) for s in (3, 4)]), None),
    ]
    return out


def by_name():
    return {name: (thr, x, sts) for name, thr, x, sts in launches()}


def batches():
    """the same reads, every group of launches that shares a threshold and a length as ONE launch: (threshold, reads)"""
    groups = {}
    for name, thr, x, _ in launches():
        groups.setdefault((float(thr), x.shape[1]), []).append(x)
    return [(thr, np.concatenate(xs)) for (thr, _), xs in sorted(groups.items())]


def run_plain(fcd, beam):
    for name, thr, x, _ in launches():
        RC.check_plain(fcd, x, beam, thr, what=name)


def run_crf(fcd, beam):
    for name, thr, x, _ in launches():
        xs, init = HS.crf_twin(x)
        RC.check_crf(fcd, xs, init, beam, thr, what=name)


def run_plain_batched(fcd, beam):
    for thr, x in batches():
        RC.check_plain(fcd, x, beam, thr, what="threshold %g, %d rows" % (thr, x.shape[1]))


def run_crf_batched(fcd, beam):
    for thr, x in batches():
        xs, init = HS.crf_twin(x)
        RC.check_crf(fcd, xs, init, beam, thr, what="threshold %g, %d rows" % (thr, x.shape[1]))
