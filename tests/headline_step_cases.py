"""TEST INFRASTRUCTURE: launches for one time step of the headline beam kernels (two reads per wavefront, reads of one
length, float32, beam 5, N = 5; csrc/beam_wave_step.inc, the HL forms: lane addresses kept as byte addresses, "this half
still runs" as a wave-uniform mask, the rank in one accumulator, new node ids by prefix count, the packed hand-over word).
Shared by tests/test_headline_step_emu.py (CPU, emulated kernels) and tests/test_gpu_headline_step.py.

Every read is compared with the oracle exactly -- labels, path, out_len, status -- under both tie orders.
  random launches: 2, 3 and 8 reads (an odd count leaves a half without a read) of T = 1, 2, 7, 65 and 130 rows -- below,
    at and past the six-row FIFO block and the 64-deep traceback segments --, reference-style rows (L2-normalised
    uniform) and peaky rows (softmax of 4 N(0, 1)), for S = 0 and for the CRF twin with S = 4;
  crafted launches, T <= 40 (table CRAFTED): each is named after the branch of the step it is made to reach, and
    reaches(name, ...) says from the reference's search alone (tests/naive_reference.py, the oracle) whether it does."""
import numpy as np

import headline_replay_cases as HC
import rank32_cases as RC
import session_cases as SC

N = 5
S = 4
BEAM = 5
THR = 0.1       # the benchmark's threshold
COUNTS = (2, 3, 8)
LENGTHS = (1, 2, 7, 65, 130)
STYLES = ("reference", "peaky")


def rows(style, seed, shape):
    """`shape` + (N,) posterior rows of the benchmark's two generators"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if style == "reference":
        x = rng.random((n, N), dtype=np.float32)
        x /= np.linalg.norm(x, ord=2, axis=1, keepdims=True)
    else:
        x = 4.0 * rng.standard_normal((n, N), dtype=np.float32)
        x -= x.max(axis=1, keepdims=True)
        np.exp(x, out=x)
        x /= x.sum(axis=1, keepdims=True)
    return np.ascontiguousarray(x.reshape(tuple(shape) + (N,)).astype(np.float32))


def random_launches():
    """(name, reads): every read count with every length, both styles"""
    out = []
    for style in STYLES:
        for T in LENGTHS:
            for B in COUNTS:
                out.append(("%s T=%d B=%d" % (style, T, B), rows(style, 1000 * T + B, (B, T))))
    return out


def random_crf_launches():
    """(name, reads, init): the same shapes with 4 states; init rows of three kinds (one-hot, random, all equal)"""
    out = []
    for style in STYLES:
        for T in LENGTHS:
            for B in COUNTS:
                x = rows(style, 2000 * T + B, (B, T, S))
                init = np.random.default_rng(T + B).random((B, S), dtype=np.float32)
                init[0] = 0.0
                init[0, (T + B) % S] = 1.0
                init[-1] = 0.25
                out.append(("crf %s T=%d B=%d" % (style, T, B), x, np.ascontiguousarray(init)))
    return out


# ---- crafted reads ---------------------------------------------------------------------------------------------------
T_CRAFT = 40
REENTRY_SEED = 11  # (asserted in the CPU test: a node leaves the beam and comes back within T_CRAFT rows)


def threshold_rows(T=T_CRAFT):
    """rows of k / 4: with thr = 0.25 a blank of exactly thr does NOT pass (pr0 > thr) and a label of exactly thr DOES
    (skipped only when pk < thr)"""
    return RC.quantised(21, T)


def under_threshold(T=24, t0=11):
    x = RC.plain_random(22, T)
    x[t0] = 0.01
    return x


def denormal_and_zero(T=T_CRAFT):
    """+0.0, -0.0 and subnormal entries next to ordinary ones, threshold 0: zeros of both signs are candidates"""
    rng = np.random.default_rng(23)
    x = RC.plain_random(23, T)
    x[rng.random((T, N)) < 0.25] = 0.0
    x[rng.random((T, N)) < 0.15] = -0.0
    x[rng.random((T, N)) < 0.15] = np.float32(2.0 ** -140)
    x[:, 0] = np.abs(x[:, 0]) + np.float32(0.05)  # (a blank that always passes keeps the read alive)
    return x.astype(np.float32)


# (name, threshold, reads, expected statuses or None = all 0)
def crafted():
    q = RC.quantised
    return [
        ("equal inside the beam, across its boundary and below it", 0.0,
         np.stack([q(1, T_CRAFT), RC.two_equal(2, T_CRAFT), q(3, T_CRAFT)]), None),
        ("a row under the threshold", 0.05, np.stack([RC.plain_random(24, 24), under_threshold()]), (0, 1)),
        ("a lone NaN", 0.5, np.stack([RC.lone_nan(0x7FC00000), RC.lone_nan(0xFFFFFFFF), RC.lone_nan(0xFFC00001)]), None),
        ("a NaN among several", 0.0, np.stack([RC.nan_among(), RC.plain_random(33, 12), RC.nan_among()]), (2, 0, 2)),
        ("zeros of both signs and denormals", 0.0,
         np.stack([RC.zero_cols(1, T_CRAFT), RC.subnormal(1, T_CRAFT), denormal_and_zero(), RC.zero_cols(2, T_CRAFT)]), None),
        ("a node re-enters the beam", THR, np.stack([rows("reference", REENTRY_SEED, (T_CRAFT,)), rows("reference", 5, (T_CRAFT,))]), None),
        ("more than 20 candidates and a tie", 0.0, np.stack([RC.constant(T_CRAFT), RC.plain_random(12, T_CRAFT), RC.constant(T_CRAFT)]), None),
        ("threshold equal to row values", 0.25, np.stack([threshold_rows(), q(25, T_CRAFT)]), None),
    ]


def _answer(want):
    return want[0], [int(v) for v in want[1]], [int(v) for v in want[2]]


def statuses(x, thr):
    return tuple(SC.want_plain(x[i], BEAM, thr, True)[0] for i in range(x.shape[0]))


def reaches(name, thr, x):
    """from the reference's search alone: does the launch reach the branch it is named after?  (a string: empty = yes)"""
    if name.startswith("equal inside"):
        met = set()
        for i in range(x.shape[0]):
            met |= RC.classes_met(x[i], BEAM, thr)
        return "" if {"inside", "boundary", "below"} <= met else "classes met: %r" % sorted(met)
    if name.startswith("a row under"):
        return "" if statuses(x, thr) == (0, 1) else "statuses %r" % (statuses(x, thr),)
    if name.startswith("a lone NaN"):
        ok = statuses(x, thr) == (0,) * x.shape[0] and all(np.isnan(x[i, 0]).sum() == 1 for i in range(x.shape[0]))
        lone = all(HC.profile(x[i], BEAM, thr)[0][2] == 1 for i in range(x.shape[0]))  # the NaN is the row's one candidate
        return "" if ok and lone else "not a lone NaN"
    if name.startswith("a NaN among"):
        return "" if statuses(x, thr) == (2, 0, 2) else "statuses %r" % (statuses(x, thr),)
    if name.startswith("zeros"):
        has = (x == 0).any() and np.signbit(x[x == 0]).any() and (~np.signbit(x[x == 0])).any() and ((x != 0) & (np.abs(x) < 2.0 ** -126)).any()
        tied = any(RC.kept_tie_steps(x[i], BEAM, thr) >= 1 for i in range(x.shape[0]))
        return "" if has and tied and statuses(x, thr) == (0,) * x.shape[0] else "no signed zeros / denormals / ties"
    if name.startswith("a node re-enters"):
        back = [t for t, (_, re, _) in enumerate(HC.profile(x[0], BEAM, thr)) if re]
        return "" if back else "no node re-enters"
    if name.startswith("more than 20"):
        return "" if HC.many_tie_steps(x[0], thr) and not RC.classes_met(x[1], BEAM, thr) else "no tie among more than 20"
    if name.startswith("threshold equal"):
        # the values are there, and each side of the asymmetry changes the answer: a threshold one ulp lower lets the blanks of
        # exactly thr pass, one ulp higher skips the labels of exactly thr
        t = np.float32(thr)
        lo, hi = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))
        here = SC.want_plain(x[0], BEAM, t, True)
        ok = (x[0][:, 0] == t).any() and (x[0][:, 1:] == t).any()
        ok = ok and _answer(SC.want_plain(x[0], BEAM, lo, True)) != _answer(here) and _answer(SC.want_plain(x[0], BEAM, hi, True)) != _answer(here)
        return "" if ok else "the threshold does not decide anything"
    return "unknown case %r" % name


def run_random(fcd):
    for name, x in random_launches():
        RC.check_plain(fcd, x, BEAM, THR, what=name)


def run_random_crf(fcd):
    for name, x, init in random_crf_launches():
        RC.check_crf(fcd, x, init, BEAM, 0.0, what=name)


def run_crafted(fcd):
    for name, thr, x, _ in crafted():
        RC.check_plain(fcd, x, BEAM, thr, what=name)
