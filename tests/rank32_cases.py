"""TEST INFRASTRUCTURE: constructed inputs for the rank on the 32-bit probability word of the two-reads-per-wavefront beam
kernels (csrc/beam_wave_step.inc, R32: candidates of equal probability share a rank, the survivor table shows when two
KEPT ones met, and only then the step recounts exact ranks with the node word).  Shared by tests/test_rank32_emu.py (CPU,
emulated kernels) and tests/test_gpu_rank32.py.

Every read is compared with the oracle: status, out_len, labels, path -- under both tie orders.  Reads (N = 5, T <= 96):
  quantised(seed)   rows of k / 4, k in 1 .. 3, unnormalised (exact in binary16 too): equal products everywhere;
  two_equal(seed)   random rows whose columns 1 and 2 (and, every third row, 3 and 4) are equal: tied children;
  constant()        all-equal rows: from the third step on more than 20 candidates, all kept ones equal (PDQ handover);
  zero_cols(seed)   columns 2 .. 4 are +0.0 or -0.0 under threshold 0: many-way ties at probability zero that reach
                    the kept ranks and the beam boundary;
  subnormal(seed)   quantised rows scaled by 2^-130: equal subnormal candidates;
  plain_random(seed) no two candidates ever equal (checked): the half that must NOT take the branch;
  lone NaN (incl. the negative NaN with an all-ones payload, whose probability word is 0), a NaN among several
  candidates (IncomparableValues), a row nothing passes (RanOutOfBeam).
tie_profile() follows the reference's search (tests/naive_reference.py) and says, per step, where equal probabilities sit
in the sorted candidate list: the tests assert from it (and from the oracle's tie counters) that a case really meets the
ties it is named after."""
import numpy as np

import naive_reference as NV
import nbest_reference as NR
import session_cases as SC
from oracle import oracle

N = 5
T = 48
BEAMS = (5, 3)
CLASSES = ("top", "inside", "boundary", "below")


def quantised(seed, T=T):
    return (np.random.default_rng(seed).integers(1, 4, size=(T, N)) / 4.0).astype(np.float32)


def two_equal(seed, T=T):
    x = np.random.default_rng(seed).random((T, N), dtype=np.float32)
    x /= x.sum(-1, keepdims=True)
    x[:, 2] = x[:, 1]
    x[::3, 4] = x[::3, 3]
    return x.astype(np.float32)


def constant(T=T):
    return np.full((T, N), 0.2, np.float32)


def zero_cols(seed, T=T):
    rng = np.random.default_rng(seed)
    x = rng.random((T, N), dtype=np.float32)
    x[:, 2:] = 0.0
    x[rng.random((T, N)) < 0.3] *= -1.0  # (-0.0 where the value is zero; negative posteriors elsewhere: below every zero)
    x[:, 0] = np.abs(x[:, 0])
    x[:, 1] = np.abs(x[:, 1])
    return x.astype(np.float32)


def subnormal(seed, T=T):
    return (quantised(seed, T) * np.float32(2.0 ** -130)).astype(np.float32)


def plain_random(seed, T=T):
    x = np.random.default_rng(seed).random((T, N), dtype=np.float32)
    return (x / x.sum(-1, keepdims=True)).astype(np.float32)


def lone_nan(bits, T=3):
    """the first row's only candidate is a NaN (threshold 0.5): never compared, the step succeeds"""
    x = np.full((T, N), 0.1, np.float32)
    x[:, 0] = 0.0
    x[0, 1] = np.array([bits], np.uint32).view(np.float32)[0]
    x[1:, 1] = 0.7
    return x


def nan_among(T=12):
    x = plain_random(31, T)
    x[T // 2, 3] = np.nan
    return x


def nothing_passes(T=12):
    x = plain_random(32, T)
    x[T // 2] = 0.01
    return x


def tie_profile(x, beam, thr, collapse=True):
    """per step of the reference's search (equal probabilities in ascending node order), the set of places where two
    neighbours of the sorted candidate list are equal: "top" ranks 0 / 1, "inside" both kept and not 0 / 1, "boundary"
    ranks beam - 1 / beam, "below" both dropped; plus "many" when a kept one ties among more than 20 candidates.
    Stops at the step that fails."""
    thr = NV.f32(thr)
    rows = [[float(v) for v in r] for r in np.asarray(x, np.float32)]
    tree = NV.SuffixTree(N - 1)
    cur = [NV.Point1(NV.ROOT_NODE, 0, 0.0, 1.0)]
    steps = []
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
        try:
            srt = NV.sort_by_probability_desc(merged, NV.Point1.probability)
        except NV.SearchError:
            break
        if not srt:
            break
        p = [c.probability() for c in srt]
        here = set()
        for j in range(len(p) - 1):
            if p[j] == p[j + 1]:
                here.add("top" if j == 0 else "inside" if j + 1 < beam else "boundary" if j + 1 == beam else "below")
                if j < beam and len(p) > 20:
                    here.add("many")
        steps.append(here)
        cur = srt[:beam]
        top = cur[0].probability()
        for c in cur:
            c.label_prob = NV.f32_div(c.label_prob, top)
            c.gap_prob = NV.f32_div(c.gap_prob, top)
    return steps


def kept_tie_steps(x, beam, thr):
    """steps in which the kernel's clash branch must fire: equal probabilities with at least one member kept"""
    return sum(1 for s in tie_profile(x, beam, thr) if s & {"top", "inside", "boundary"})


def classes_met(x, beam, thr):
    out = set()
    for s in tie_profile(x, beam, thr):
        out |= s
    return out


# ---- the launches: (name, threshold, reads) -- 2 .. 8 reads each ----------------------------------------------------
def tied_launches():
    """every read of these meets a kept tie (asserted in the CPU test for both beams)"""
    return [
        ("quantised", 0.0, np.stack([quantised(s) for s in (1, 2, 3, 4, 5, 6)])),   # three wavefronts, both halves tied
        ("quantised thr", 0.3, np.stack([quantised(s) for s in (7, 8)])),
        ("two equal columns", 0.05, np.stack([two_equal(s) for s in (1, 2, 3)])),   # the last wavefront has one read
        ("constant", 0.0, np.stack([constant(), np.float32(0.5) * constant()])),
        ("zero columns", 0.0, np.stack([zero_cols(s) for s in (1, 2, 3, 4)])),
        ("subnormal", 0.0, np.stack([subnormal(s) for s in (1, 2)])),
    ]


def half_launches():
    """two reads of one wavefront: which half meets kept ties -- (name, thr, reads, (first half tied, second half tied))"""
    q, r = quantised(11), plain_random(12)
    return [
        ("both halves", 0.0, np.stack([q, quantised(13)]), (True, True)),
        ("first half only", 0.0, np.stack([q, r]), (True, False)),
        ("second half only", 0.0, np.stack([r, q]), (False, True)),
    ]


def failing_launches():
    """(name, thr, reads, statuses): the lone NaNs succeed, a NaN among several and an empty list fail"""
    lone = np.stack([lone_nan(0x7FC00000), lone_nan(0xFFFFFFFF), lone_nan(0xFFC00001), lone_nan(0x7FFFFFFF)])
    return [
        ("lone NaN", 0.5, lone, None),
        ("NaN among several", 0.0, np.stack([nan_among(), plain_random(33, 12), quantised(34, 12)]), (2, 0, 0)),
        ("nothing passes", 0.05, np.stack([quantised(35, 12), nothing_passes()]), (0, 1)),
    ]


def crf_launch(S=4, T=40):
    """CRF, 4 states: quantised rows and a constant read; every read meets a tie the oracle counts as critical"""
    rng = np.random.default_rng(41)
    x = (rng.integers(1, 4, size=(4, T, S, N)) / 4.0).astype(np.float32)
    x[3] = 0.25
    init = np.ascontiguousarray(np.tile(np.array([0.1, 0.6, 0.2, 0.1], np.float32), (4, 1)))
    init[2] = 0.25  # (an all-equal init row: the first maximum wins)
    return np.ascontiguousarray(x), init


# ---- runners --------------------------------------------------------------------------------------------------------
def check_plain(fcd, x, beam, thr, lengths=None, what=""):
    r = fcd.beam_search_batch_raw(np.ascontiguousarray(x), beam, thr, True, lengths=lengths, kernel=SC.KERNEL_WAVE).cpu()
    xf = np.asarray(x).astype(np.float32)
    for i in range(xf.shape[0]):
        Ti = xf.shape[1] if lengths is None else int(lengths[i])
        SC.check_slot(r, i, SC.want_plain(xf[i, :Ti], beam, thr, True), "%s beam %d read %d" % (what, beam, i))
    return r


def check_crf(fcd, x, init, beam, thr, what=""):
    r = fcd.crf_beam_search_batch_raw(x, init, beam, thr, kernel=SC.KERNEL_WAVE).cpu()
    for i in range(x.shape[0]):
        SC.check_slot(r, i, SC.want_crf(x[i], init[i], beam, thr), "%s crf beam %d read %d" % (what, beam, i))
    return r


def run_session(fcd, x, beam, thr, to_input=None, host=True):
    """row by row: the saved state carries every lane's candidate across launches; every prefix against the oracle"""
    conv = to_input or (lambda a: a)
    B, Tn = x.shape[:2]
    with fcd.BeamSearchSession(B, N, Tn, beam, thr, True, kernel=SC.KERNEL_WAVE) as s:
        for t in range(Tn):
            r = s.push(conv(np.ascontiguousarray(x[:, t:t + 1])), result=True).cpu()
            for i in range(B):
                SC.check_slot(r, i, SC.want_plain(x[i, :t + 1], beam, thr, True), "session row %d" % t)
        final = s.result(host=host).cpu()
    one = fcd.beam_search_batch_raw(conv(x), beam, thr, True, kernel=SC.KERNEL_WAVE).cpu()
    SC.same_result(final, one, "session vs one-shot")


def run_nbest(fcd, x, beam, thr, stable, lengths=None, to_input=None):
    import nbest_cases as NC
    xin = x if to_input is None else to_input(x)
    B = x.shape[0]
    lens = [x.shape[1]] * B if lengths is None else [int(v) for v in lengths]
    r = fcd.beam_search_nbest_batch_raw(xin, beam, beam, thr, lengths=lengths, kernel=SC.KERNEL_WAVE).cpu()
    want = [NR.beam_search(x[i, :lens[i]], beam, thr, True, stable=stable) for i in range(B)]
    NC.check(r, want, beam, B)


def counted(x, beam, thr):
    """the oracle's two tie counters of a read: (kept tie among more than 20, tie at ranks 0 / 1 or across the boundary)"""
    return tuple(int(v) for v in oracle.beam_search_ambiguous(np.ascontiguousarray(x), beam, thr, True)[3])
