"""TEST INFRASTRUCTURE: constructed inputs for the renormalising divisions of the two-reads-per-wavefront beam kernels
(csrc/beam_wave_step.inc, DSRC: every candidate is divided by the top probability on the lane it sits on, the quotients
are gathered -- a slot's gap quotient from its source group's spare lane, or, for a child candidate, 0 / top from an idle
lane of the half).  Shared by tests/test_divide_source_emu.py (CPU, emulated kernels) and tests/test_gpu_divide_source.py.

Reads, grouped by the threshold they need (a launch has one):
  0.1: (a) a new label beats the blank in every step: a child candidate takes rank 0, the slot's own candidate survives below;
       (b) own candidates with a gap but no label probability (the root; a blank row whose tip fails the threshold) and with
           a label but no gap probability (a repeat whose blank fails the threshold);
       a random read;
  0.0: (c) all-zero rows: every candidate 0, top == 0, the quotients NaN;
       (e) rows scaled by 2^-120: subnormal candidates and divisor;
       (f) constant rows: from the third step on 21 or more candidates, all kept ones equal (the quicksort's tie order:
           the step settles twice);
  0.5: (d) a NaN label next to labels below the threshold: the read's lone candidate is NaN and is never compared;
       two random reads.
Every case is compared with the oracle: status, out_len, labels, path."""
import numpy as np

import session_cases as SC
from oracle import oracle

N = 5
TS = (1, 2, 7, 65)
BEAMS = (1, 2, 3, 4, 5)
THRS = (0.1, 0.0, 0.5)


def _random(seed, T):
    x = np.random.default_rng(seed).random((T, N), dtype=np.float32)
    return (x / x.sum(-1, keepdims=True)).astype(np.float32)


def child_on_top(T):
    x = np.full((T, N), 0.025, np.float32)
    x[:, 0] = 0.3
    x[np.arange(T), 1 + np.arange(T) % 4] = 0.6
    return x


def gap_only_label_only(T):
    x = np.empty((T, N), np.float32)
    x[0::2] = [0.05, 0.8, 0.1, 0.03, 0.02]   # blank below the threshold: a repeat of label 1 keeps its label probability only
    x[1::2] = [0.5, 0.02, 0.02, 0.4, 0.06]   # the tip fails the threshold: the blank alone keeps the entry
    return x


def zeros(T):
    return np.zeros((T, N), np.float32)


def subnormal(T):
    x = _random(11, T)
    x[:, 2] /= 64.0
    x[:, 4] /= 1024.0
    return (x * np.float32(2.0 ** -120)).astype(np.float32)


def constant(T):
    return np.full((T, N), 0.2, np.float32)


def lone_nan(T):
    x = np.full((T, N), 0.1, np.float32)
    x[:, 0] = 0.0
    x[0, 1] = np.nan
    x[1:, 1] = 0.7
    return x


def group(thr, T):
    """the (3, T, N) reads of threshold `thr`"""
    if thr == 0.1:
        reads = [child_on_top(T), gap_only_label_only(T), _random(3, T)]
    elif thr == 0.0:
        reads = [zeros(T), subnormal(T), constant(T)]
    else:
        reads = [lone_nan(T), _random(5, T), _random(6, T)]
    return np.ascontiguousarray(np.stack(reads).astype(np.float32))


def crf_group(thr, T, S=4):
    """the CRF twins of (a) and (c) (and a random read): every state sees the plain read's row"""
    plain = [child_on_top(T), zeros(T), _random(7, T)] if thr == 0.0 else [child_on_top(T), _random(8, T), _random(9, T)]
    x = np.stack([np.repeat(p[:, None, :], S, axis=1) for p in plain]).astype(np.float32)
    rng = np.random.default_rng(21)
    x[2] = rng.random((T, S, N), dtype=np.float32)
    init = np.ascontiguousarray(np.tile(np.array([0.1, 0.6, 0.2, 0.1], np.float32), (3, 1)))
    return np.ascontiguousarray(x), init


def check_plain(fcd, x, beam, thr, n_reads, first=0, count_ambiguous=False, lengths=None, what=""):
    """reads first .. first + n_reads - 1 of x in one launch (3 reads leave the second wavefront an empty half)"""
    sub = np.ascontiguousarray(x[first:first + n_reads])
    r = fcd.beam_search_batch_raw(sub, beam, thr, True, lengths=lengths, kernel=SC.KERNEL_WAVE,
                                  count_ambiguous=count_ambiguous).cpu()
    xf = sub.astype(np.float32)
    for i in range(n_reads):
        T = xf.shape[1] if lengths is None else int(lengths[i])
        SC.check_slot(r, i, SC.want_plain(xf[i, :T], beam, thr, True), "%s thr %g beam %d read %d" % (what, thr, beam, first + i))
    return r


def check_crf(fcd, x, init, beam, thr, n_reads, first=0, what=""):
    sub, ini = np.ascontiguousarray(x[first:first + n_reads]), np.ascontiguousarray(init[first:first + n_reads])
    r = fcd.crf_beam_search_batch_raw(sub, ini, beam, thr, kernel=SC.KERNEL_WAVE).cpu()
    for i in range(n_reads):
        SC.check_slot(r, i, SC.want_crf(sub[i], ini[i], beam, thr), "%s crf thr %g beam %d read %d" % (what, thr, beam, first + i))
    return r


def run_shapes(fcd, T, beam):
    """every group at (T, beam): 1 read (a different one per shape) and 3 reads; the CRF twins"""
    for thr in THRS:
        x = group(thr, T)
        check_plain(fcd, x, beam, thr, 1, first=(T + beam) % 3, what="T %d" % T)
        check_plain(fcd, x, beam, thr, 3, what="T %d" % T)
    for thr in (0.1, 0.0):
        x, init = crf_group(thr, T)
        check_crf(fcd, x, init, beam, thr, 1, first=(T + beam) % 2, what="T %d" % T)
        check_crf(fcd, x, init, beam, thr, 3, what="T %d" % T)


def run_variants(fcd, T, beam):
    """the other instantiations of the family: 16-bit posteriors, ragged lengths, the tie counters"""
    x = group(0.1, T)
    check_plain(fcd, x.astype(np.float16), beam, 0.1, 3, what="f16")
    lengths = np.array([T, max(T - 1, 0), (T + 1) // 2], np.int64)
    for thr in THRS:
        check_plain(fcd, group(thr, T), beam, thr, 3, lengths=lengths, what="ragged")
        check_plain(fcd, group(thr, T), beam, thr, 3, count_ambiguous=True, what="counted")


def tied_steps(T, beam):
    """how many steps of the constant read keep a candidate that ties among more than 20 (the oracle's counter)"""
    return int(oracle.beam_search_ambiguous(constant(T), beam, 0.0, True)[3][0])


def run_session(fcd, thr, T, beam, to_input=None, host=True):
    """1-row pushes: the stored quotients are written and read back at every row; every prefix against the oracle, the end
    against the one-shot launch"""
    x = group(thr, T)
    conv = to_input or (lambda a: a)
    with fcd.BeamSearchSession(3, N, T, beam, thr, True, kernel=SC.KERNEL_WAVE) as s:
        for t in range(T):
            r = s.push(conv(np.ascontiguousarray(x[:, t:t + 1])), result=True).cpu()
            for i in range(3):
                SC.check_slot(r, i, SC.want_plain(x[i, :t + 1], beam, thr, True), "session thr %g row %d" % (thr, t))
        final = s.result(host=host).cpu()
    one = fcd.beam_search_batch_raw(conv(x), beam, thr, True, kernel=SC.KERNEL_WAVE).cpu()
    SC.same_result(final, one, "session vs one-shot")
