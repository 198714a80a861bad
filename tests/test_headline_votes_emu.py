"""CPU-side check of the wave-wide votes of the headline beam kernels (csrc/beam_wave_step.inc, the HL family: lane
predicates formed as masks, votes on bare compares joined in scalar registers) on tests/hipemu's lockstep emulation: the
constructed reads of tests/headline_votes_cases.py against the oracle -- labels, path, out_len and status, exactly, under
both tie orders, beams 5 and 3, over N = 3, 4, 5 and the CRF twin with 4 states.
The first tests establish, from the reference's own search, that the crafted reads reach the states they are named
after.  The emulator aborts when a node re-enters the beam and its child row was never stored ("row never stored"): a
wrong eviction mask ends the run.
test_guard_flags_the_same_words builds a small stand-alone program that walks all 2^32 probabilities and compares the
guard as the step votes it (device_utils.h, fcd_rankf_outside_a: three compares of the probability and of the count's own
term) with fcd_rankf_outside() on the probability's word."""
import os
import subprocess

import numpy as np
import pytest

import headline_votes_cases as HV
import rank32_cases as RC
import rank_domain_cases as DC
from emu_util import emulated_kernels
from tie_util import ORDERS, tie_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVENTS = {"followed", "entered", "reentered", "evicted_live", "evicted_dead"}

GUARD_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "device_utils.h"
int main() {
    unsigned long long bad = 0, flagged = 0;
    for (unsigned long long b = 0; b < (1ull << 32); ++b) {
        const uint32_t bits = (uint32_t)b;
        float p;
        memcpy(&p, &bits, 4);
        const uint32_t word = (uint32_t)(fcd::make_key(p, 0) >> 32);
        const bool was = fcd::fcd_rankf_outside(word);
        const bool now = fcd::fcd_rankf_outside_a(p, fcd::fcd_rankf_own(word), fcd::kRankfALo, fcd::kRankfAHi);
        if (was != now && bad++ < 8) printf("differs: p bits %08x word %08x was %d now %d\n", bits, word, (int)was, (int)now);
        flagged += now;
    }
    printf("bad %llu flagged %llu\n", bad, flagged);
    return bad != 0;
}
"""


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


def test_guard_flags_the_same_words(tmp_path):
    src = tmp_path / "guard_walk.cpp"
    exe = tmp_path / "guard_walk"
    src.write_text(GUARD_PROGRAM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-w", "-DFCD_HIPEMU=1",
                           "-I", os.path.join(ROOT, "tests", "hipemu"), "-I", os.path.join(ROOT, "fast_ctc_decode_amd", "csrc"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1].split()
    bad, flagged = int(last[1]), int(last[3])
    assert bad == 0
    # the accepted probabilities: +0 and -0 and the finite ones in [2^-76, 2^27]
    lo, hi = int(np.float32(2.0 ** -76).view(np.uint32)), int(np.float32(2.0 ** 27).view(np.uint32))
    assert flagged == 2 ** 32 - (hi - lo + 1) - 2


def test_the_reads_reach_the_states_they_are_named_after():
    for beam in HV.BEAMS:
        # halves: the failing read ends on its second step, its neighbour runs to the end
        for name, thr, x in HV.halves_launches()[2:]:
            n = [len(HV.step_profile(x[i], beam, thr)) for i in (0, 1)]
            first = name.startswith("first")
            assert n == ([2, x.shape[1]] if first else [x.shape[1], 2]), (name, beam, n)
            st = [RC.SC.want_plain(x[i], beam, thr, True)[0] for i in (0, 1)]
            assert (st[0] != 0, st[1] != 0) == (first, not first), (name, beam, st)
        # numbering: the first step holds the root alone; blank-only rows create nothing; a full beam of fresh leaves
        # creates a node on every child lane
        name, thr, x = HV.numbering_launches()[0]
        for i in (0, 1):
            p = HV.step_profile(x[i], beam, thr)
            assert p[0]["n_cand"] <= HV.N and p[0]["n_new"] >= 1, (beam, i)
            zero = [s["n_new"] == 0 for s in p]
            assert sum(zero) >= 6 and any(s["n_new"] > 0 for s in p[zero.index(True) + 6:]), (beam, i)
            assert all(s["n_cand"] >= 1 for s in p)
        p = HV.step_profile(HV.twenty_new(), beam, 0.05)
        assert p[2]["n_new"] == 0 and p[3]["n_new"] == beam * (HV.N - 1) and p[3]["n_cand"] == beam * HV.N, (beam, p[:4])
        # both votes rise in one step
        for name, thr, x in HV.both_votes_launches():
            assert all(HV.both_votes_steps(x[i], beam, thr) >= 1 for i in range(x.shape[0])), (name, beam)
        # child fate: all five events, in one read
        for s in HV.FATE_SEEDS[:3]:
            assert HV.met(RC.plain_random(s), beam, 0.05) == EVENTS, (beam, s)
    assert HV.step_profile(HV.twenty_new(), 5, 0.05)[3]["n_new"] == 20


def test_the_domain_tables_keep_their_doors_on_the_other_members():
    """cut to 3 or 4 columns, or spread over 4 CRF states, the OUTSIDE reads still hold a candidate outside the domain and
    the INSIDE ones none (the CRF search has no repeat-stay, so its candidates are followed with collapse off)"""
    for n in (3, 4):
        for name, thr, x in DC.inside_launches():
            xs = HV.small_alphabet(x, n)
            assert not any(any(DC.outside_steps(xs[i], 5, thr)) for i in range(xs.shape[0])), (n, name)
        for name, thr, x, _ in DC.outside_launches():
            xs = HV.small_alphabet(x, n)
            if n == 3 and name in ("one column 2^-80", "one column 2^30", "one column 2^40", "negative posteriors"):
                continue  # (the column they scale is cut off)
            assert all(any(DC.outside_steps(xs[i], 5, thr)) for i in range(xs.shape[0])), (n, name)
    for name, thr, x in DC.inside_launches():
        assert not any(any(DC.outside_steps(x[i], 5, thr, collapse=False)) for i in range(x.shape[0])), name
    for name, thr, x, _ in DC.outside_launches():
        assert all(any(DC.outside_steps(x[i], 5, thr, collapse=False)) for i in range(x.shape[0])), name


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", HV.BEAMS)
def test_plain(fcd, order, beam):
    with tie_order(fcd, order):
        HV.run_plain(fcd, beam)


@pytest.mark.parametrize("n", (3, 4))
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", HV.BEAMS)
def test_small_alphabets(fcd, order, beam, n):
    with tie_order(fcd, order):
        HV.run_small(fcd, beam, n)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", HV.BEAMS)
def test_crf_twin(fcd, order, beam):
    with tie_order(fcd, order):
        HV.run_crf(fcd, beam)
