"""TEST INFRASTRUCTURE: launches for the loop-carried forms of the headline beam kernels (csrc/beam_wave.hip and
csrc/beam_wave_step.inc, the HL family: two reads per wavefront, reads of one length, float32, N = 5, S = 0 and the CRF twin
with S = 4): the row FIFO's refill address carried as a running 64-bit lane address, the per-half candidate counts and the
mask of the beam's groups, the divisor read from the survivor table as the probability the source lane stored, the depth
carried shifted.  Shared by tests/test_headline_loop_emu.py (CPU, emulated kernels) and tests/test_gpu_headline_loop.py.

Every launch has at most 8 reads of at most 130 rows and is compared with the oracle exactly -- labels, path, out_len,
status -- under both tie orders.
  refill: S = 0 holds six rows per FIFO register and 42 rows in flight: lengths 1, 5, 6, 7, 41, 42, 43, 48, 49, 85 with 1, 2
    and 3 reads (an odd count leaves a half without a read), each contiguous and on a view with a padded stride_t, stride_n = 2
    and a read stride larger than the read -- everything outside the view is NaN, so a wrong address changes the answer.  The
    S = 4 twin holds one row per register: lengths 1, 2, 6, 7, 8, 43.  The N = 3 and N = 4 members hold ten and eight rows per
    register: the lengths around one register and around the seven in flight.
  per-half counts: a peaky read next to a reference-style read, a read that runs out of beam at a known row next to a healthy
    one, a read with a NaN among several candidates next to a healthy one -- each in both half orders, beams 1 .. 5, collapse
    on and off, thresholds 0 and 0.1.
  divisor: threshold 0 with an all-zero row (the top probability is 0), rows holding -0.0, zeros of both signs next to
    denormals, ranks 0 and 1 tied among more than 20 candidates.
reaches(...) says from the reference's search alone (tests/naive_reference.py, the oracle) whether a crafted launch reaches the
case it is named after."""
import numpy as np

import headline_replay_cases as HC
import headline_step_cases as HS
import headline_votes_cases as HV
import rank32_cases as RC
import session_cases as SC

N = 5
S = 4
THR = 0.1
REFILL_LENGTHS = (1, 5, 6, 7, 41, 42, 43, 48, 49, 85)
REFILL_LENGTHS_S4 = (1, 2, 6, 7, 8, 43)
COUNTS = (1, 2, 3)
BEAMS = (1, 2, 3, 4, 5)
THRS = (0.0, 0.1)
T_OUT = 11  # the row at which the failing reads end


def padded_view(x):
    """the same values on a view of a larger array: stride_n = 2, a padded stride_t, a read stride larger than the read; NaN
    everywhere else"""
    x = np.asarray(x, np.float32)
    shape = x.shape[:1] + (x.shape[1] + 2,) + x.shape[2:-1] + (2 * x.shape[-1] + 3,)
    base = np.full(shape, np.nan, np.float32)
    v = base[:, :x.shape[1], ..., 0:2 * x.shape[-1]:2]
    v[...] = x
    assert v.shape == x.shape and not v.flags["C_CONTIGUOUS"]
    return v


def refill_launches():
    """(name, reads): reference-style rows, every length with every read count"""
    return [("refill T=%d B=%d" % (T, B), HS.rows("reference", 3000 * T + B, (B, T))) for T in REFILL_LENGTHS for B in COUNTS]


def small_lengths(n):
    """N = 3 and 4 hold 32 // N rows per FIFO register and seven registers in flight: the lengths around both"""
    rpr = 32 // n
    return (1, rpr - 1, rpr, rpr + 1, 7 * rpr - 1, 7 * rpr, 7 * rpr + 1, 8 * rpr + 1)


def refill_small_launches(n):
    """(name, reads): the N = 3 and N = 4 members of the family -- reference-style rows cut to n columns"""
    return [("refill N=%d T=%d B=%d" % (n, T, B), np.ascontiguousarray(HS.rows("reference", 5000 * T + B + n, (B, T))[:, :, :n]))
            for T in small_lengths(n) for B in COUNTS]


def all_launches():
    """every array this file launches (the size bound is asserted on them in the CPU test)"""
    out = [x for _, x in refill_launches()] + [x for _, x, _ in refill_crf_launches()] + [x for _, x in half_launches()]
    out += [x for _, _, x in divisor_launches()] + [x for n in (3, 4) for _, x in refill_small_launches(n)]
    return out


def refill_crf_launches():
    out = []
    for T in REFILL_LENGTHS_S4:
        for B in COUNTS:
            x = HS.rows("reference", 4000 * T + B, (B, T, S))
            init = np.random.default_rng(7 * T + B).random((B, S), dtype=np.float32)
            out.append(("refill crf T=%d B=%d" % (T, B), x, np.ascontiguousarray(init)))
    return out


# ---- per-half counts -------------------------------------------------------------------------------------------------
def runs_out(T=24, t0=T_OUT):
    """plain rows; row t0 is negative throughout: the blank is not above and every label is below either threshold"""
    x = RC.plain_random(52, T)
    x[t0] = -1.0
    return x


def nan_read(T=24, t0=T_OUT):
    """plain rows of which every entry passes both thresholds; a NaN among them in row t0 (it passes: `pb < thr` is false)"""
    x = (RC.plain_random(53, T) + np.float32(0.15)).astype(np.float32)
    x[t0, 3] = np.nan
    return x


def half_launches():
    """(name, reads): the odd read first and second"""
    peaky, ref = HS.rows("peaky", 61, (24,)), HS.rows("reference", 62, (24,))
    healthy = (RC.plain_random(54, 24) + np.float32(0.15)).astype(np.float32)
    out = []
    for name, odd, other in (("peaky", peaky, ref), ("runs out", runs_out(), healthy), ("nan", nan_read(), healthy)):
        out.append((name + " first", np.stack([odd, other])))
        out.append((name + " second", np.stack([other, odd])))
    return out


def counts_differ(x, beam, thr, collapse):
    """the candidate counts of the two reads, step by step, are not the same list"""
    a, b = ([s["n_cand"] for s in HV.step_profile(x[i], beam, thr, collapse)] for i in (0, 1))
    return a != b


def half_reaches(name, x, beam, thr, collapse):
    """empty string = the launch reaches what it is named after"""
    st = tuple(SC.want_plain(x[i], beam, thr, collapse)[0] for i in (0, 1))
    odd = 0 if name.endswith("first") else 1
    if name.startswith("peaky"):
        # (one cell of the grid cannot part the halves: at threshold 0 every entry of a positive row passes, and with beam 1 and
        # collapse off the lone beam entry then has exactly N candidates in every step of either read.  Everywhere else -- a
        # second beam entry merges extensions with existing nodes, collapse adds the repeat-stay, threshold 0.1 drops most of
        # the peaky read's labels -- the two halves' counts must differ in some step)
        forced_equal = thr == 0.0 and beam == 1 and not collapse
        differ = forced_equal or counts_differ(x, beam, thr, collapse)
        return "" if st == (0, 0) and differ else "statuses %r or equal counts" % (st,)
    want = 1 if name.startswith("runs out") else 2
    steps = len(HV.step_profile(x[odd], beam, thr, collapse))
    ok = st[odd] == want and st[1 - odd] == 0 and steps == T_OUT + 1
    return "" if ok else "statuses %r, the odd read took %d steps" % (st, steps)


# ---- divisor ---------------------------------------------------------------------------------------------------------
def zero_row(T=24, t0=9):
    x = RC.plain_random(71, T)
    x[t0] = 0.0
    return x


def minus_zero_rows(T=24):
    x = RC.plain_random(72, T)
    x[3::4, 1:] = -0.0
    x[5, :] = -0.0
    x[5, 0] = 0.3
    return x


def divisor_launches():
    """(name, threshold, reads)"""
    return [
        ("an all-zero row", 0.0, np.stack([zero_row(), RC.plain_random(73, 24)])),
        ("rows holding -0.0", 0.0, np.stack([RC.plain_random(74, 24), minus_zero_rows(), minus_zero_rows()[::-1].copy()])),
        ("zeros of both signs and denormals", 0.0, np.stack([HS.denormal_and_zero(), RC.zero_cols(3, HS.T_CRAFT)])),
        ("ranks 0 and 1 tie among more than 20", 0.0, np.stack([RC.constant(40), RC.plain_random(75, 40), RC.constant(40)])),
    ]


def divisor_reaches(name, thr, x, beam=5):
    if name.startswith("an all-zero"):
        t0 = int(np.flatnonzero((x[0] == 0).all(axis=1))[0])
        prof = HV.step_profile(x[0], beam, thr)
        return "" if len(prof) > t0 and prof[t0]["n_cand"] >= 2 else "the read does not reach its zero row with several candidates"
    if name.startswith("rows holding"):
        z = x[1][x[1] == 0]
        return "" if z.size and np.signbit(z).all() and len(HV.step_profile(x[1], beam, thr)) == x.shape[1] else "no -0.0, or the read ends"
    if name.startswith("zeros of both"):
        z = x[0][x[0] == 0]
        ok = np.signbit(z).any() and (~np.signbit(z)).any() and ((x[0] != 0) & (np.abs(x[0]) < 2.0 ** -126)).any()
        return "" if ok else "no signed zeros / denormals"
    if name.startswith("ranks 0 and 1"):
        ok = any({"top", "many"} <= s for s in RC.tie_profile(x[0], beam, thr)) and HC.many_tie_steps(x[0], thr)
        return "" if ok else "no tie of ranks 0 and 1 among more than 20 candidates"
    return "unknown case %r" % name


# ---- runners (the caller sets the tie order) -------------------------------------------------------------------------
def check(fcd, x, beam, thr, collapse, what):
    r = fcd.beam_search_batch_raw(x, beam, thr, collapse, kernel=SC.KERNEL_WAVE).cpu()
    for i in range(x.shape[0]):
        SC.check_slot(r, i, SC.want_plain(np.ascontiguousarray(x[i]), beam, thr, collapse), "%s beam %d read %d" % (what, beam, i))


def run_refill(fcd, view):
    for name, x in refill_launches():
        check(fcd, padded_view(x) if view else x, HS.BEAM, THR, True, name + (" view" if view else ""))


def run_refill_small(fcd, n, view):
    for name, x in refill_small_launches(n):
        check(fcd, padded_view(x) if view else x, HS.BEAM, THR, True, name + (" view" if view else ""))


def run_refill_crf(fcd, view):
    for name, x, init in refill_crf_launches():
        xin = padded_view(x) if view else x
        r = fcd.crf_beam_search_batch_raw(xin, init, HS.BEAM, 0.0, kernel=SC.KERNEL_WAVE).cpu()
        for i in range(x.shape[0]):
            SC.check_slot(r, i, SC.want_crf(x[i], init[i], HS.BEAM, 0.0), "%s%s read %d" % (name, " view" if view else "", i))


def run_halves(fcd, beam, collapse):
    for thr in THRS:
        for name, x in half_launches():
            check(fcd, x, beam, thr, collapse, "%s thr %g collapse %d" % (name, thr, collapse))


def run_divisor(fcd):
    for name, thr, x in divisor_launches():
        check(fcd, x, HS.BEAM, thr, True, name)
