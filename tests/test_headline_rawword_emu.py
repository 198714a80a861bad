"""CPU-side check of the raw probability table of the headline beam kernels (csrc/beam_wave_step.inc, RAWK: the every-step
path writes and ranks bits(prob + 0.0f); keyed probability words and node words are formed, and both tables rebuilt, only
inside the step's rare block) on tests/hipemu's lockstep emulation: the launches of tests/headline_rawword_cases.py against
the oracle -- labels, path, out_len and status, exactly, under both tie orders, S = 0 and the CRF twin with 4 states.
The first tests establish, from the reference's own search and the oracle's tie counters, that every crafted read reaches
the branch it is named after; a read that does not fails the test.
test_guard_on_raw_words builds a small stand-alone program that walks all 2^32 probabilities p and compares the guard as the
step votes it now -- fcd_rankf_outside_a on p and on A = fcd_rankp_own(bits(p + 0.0f)) = -p * 2^100, for EVERY p -- with
fcd_rankf_outside() on p's keyed word, and the raw own term with the keyed one wherever the count is exact.
The -m gpu twin is tests/test_gpu_headline_rawword.py."""
import os
import subprocess

import numpy as np
import pytest

import headline_rawword_cases as HR
import rank32_cases as RC
import session_cases as SC
from emu_util import emulated_kernels
from tie_util import ORDERS, tie_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GUARD_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "device_utils.h"
int main() {
    unsigned long long bad = 0, flagged = 0, own_differs = 0, negative = 0;
    for (unsigned long long b = 0; b < (1ull << 32); ++b) {
        const uint32_t bits = (uint32_t)b;
        float p;
        memcpy(&p, &bits, 4);
        const uint32_t word = (uint32_t)(fcd::make_key(p, 0) >> 32);  // the keyed word of p
        const float pc = p + 0.0f;
        uint32_t raw;
        memcpy(&raw, &pc, 4);                                         // the raw word the table holds
        const bool was = fcd::fcd_rankf_outside(word);
        const float a = fcd::fcd_rankp_own(raw);
        const bool now = fcd::fcd_rankf_outside_a(p, a, fcd::kRankfALo, fcd::kRankfAHi);
        if (was != now && bad++ < 8) printf("differs: p bits %08x word %08x raw %08x was %d now %d\n", bits, word, raw, (int)was, (int)now);
        flagged += now;
        if (!was) {  // inside the domain the raw own term IS the keyed one, bit for bit (-0.0 for both zeros)
            const float k = fcd::fcd_rankf_own(word);
            if (memcmp(&k, &a, 4) != 0 && own_differs++ < 8) printf("own term differs: p bits %08x\n", bits);
        }
        if (p < 0.0f) {  // every negative p: A > 0, the second vote
            negative++;
            if (!(a > fcd::kRankfALo && p != 0.0f) && bad++ < 8) printf("negative p not caught by the second vote: %08x\n", bits);
        }
        if (p != p && (a >= fcd::kRankfAHi) && bad++ < 8) printf("NaN p not caught by the first vote: %08x\n", bits);
    }
    printf("bad %llu flagged %llu own_differs %llu negative %llu\n", bad, flagged, own_differs, negative);
    return bad != 0 || own_differs != 0;
}
"""


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


def test_guard_on_raw_words(tmp_path):
    src = tmp_path / "guard_walk_raw.cpp"
    exe = tmp_path / "guard_walk_raw"
    src.write_text(GUARD_PROGRAM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-w", "-DFCD_HIPEMU=1",
                           "-I", os.path.join(ROOT, "tests", "hipemu"), "-I", os.path.join(ROOT, "fast_ctc_decode_amd", "csrc"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1].split()
    bad, flagged, own_differs, negative = int(last[1]), int(last[3]), int(last[5]), int(last[7])
    assert bad == 0 and own_differs == 0
    # the accepted probabilities: +0 and -0 and the finite ones in [2^-76, 2^27]
    lo, hi = int(np.float32(2.0 ** -76).view(np.uint32)), int(np.float32(2.0 ** 27).view(np.uint32))
    assert flagged == 2 ** 32 - (hi - lo + 1) - 2
    assert negative == 0x7F800000  # -inf and every negative finite value but -0.0


def test_the_tie_reads_meet_the_pairs_they_are_named_after():
    for pair in HR.PAIRS:
        for where in ("inside", "boundary"):
            assert (pair, where) in HR.ties_met(HR.tie_read(pair, where)), (pair, where)
    for T in (1, 130):
        x = HR.dyadic(3 if T == 130 else 1, T)
        assert len(HR.report(x)) == T
    assert HR.ties_met(HR.dyadic(3, 130)) != set() and HR.ties_met(RC.constant(1)) != set()


def test_the_many_candidate_reads_replay_in_the_halves_they_are_named_after():
    by_name = {name: (thr, x) for name, thr, x, _ in HR.launches()}
    for name, halves in (("many, lower half only", (True, False)), ("many, upper half only", (False, True)),
                         ("many, both halves", (True, True))):
        thr, x = by_name[name]
        got = tuple(bool(HR.many_steps(x[i], thr)) for i in (0, 1))
        assert got == halves, (name, got)
        # the half that must not be flagged holds no kept tie at all: nothing of its step is recounted for its own sake
        for i in (0, 1):
            if not halves[i]:
                assert HR.ties_met(x[i], thr) == set(), name
    many = HR.many_steps(RC.constant(40))
    assert any(b == a + 1 for a, b in zip(many, many[1:])), many  # two such steps in a row: each rebuilds the keyed tables
    assert RC.counted(RC.constant(40), HR.BEAM, 0.0)[0] >= len(many)  # the oracle's own counter of kept ties above 20
    c, h = by_name["many, both halves"][1][0], by_name["many, both halves"][1][1]
    assert set(HR.many_steps(c)) & set(HR.many_steps(h)), "no step in which both halves replay"


def test_the_guarded_reads_hold_what_they_are_named_after():
    by_name = {name: (thr, x, sts) for name, thr, x, sts in HR.launches()}

    thr, x, _ = by_name["below 2^-76"]
    assert any(s["outside"] for s in HR.report(x[0], HR.BEAM, thr)) and not any(s["outside"] for s in HR.report(x[1], HR.BEAM, thr))
    thr, x, _ = by_name["negative"]
    for i in (0, 1):
        r = HR.report(x[i], HR.BEAM, thr)
        assert any(s["negative"] and s["outside"] for s in r), i  # two or more negative candidates: raw and keyed order differ
    assert not any(s["outside"] for s in HR.report(x[2], HR.BEAM, thr))
    thr, x, sts = by_name["a NaN"]
    got = tuple(SC.want_plain(x[i], HR.BEAM, thr, True)[0] for i in range(x.shape[0]))
    assert got == sts and HR.report(x[0], HR.BEAM, thr)[-1]["outside"], got
    thr, x, _ = by_name["+inf"]
    for i in (0, 1):  # the +inf is ranked (row 6) in a step that succeeds: the read goes on to row 7
        r = HR.report(x[i], HR.BEAM, thr)
        assert r[6]["outside"] and len(r) >= 8, (i, len(r))
    thr, x, _ = by_name["zero beside empty slots"]
    for i in (0, 1):
        r = HR.report(x[i], HR.BEAM, thr)
        assert r[0]["zero"] and r[0]["n"] == HR.N and not any(s["outside"] for s in r), i  # five candidates, twenty empty slots
    for name, (thr, x, sts) in by_name.items():
        assert x.shape[0] <= 8 and 1 <= x.shape[1] <= 130, name
        got = tuple(SC.want_plain(x[i], HR.BEAM, thr, True)[0] for i in range(x.shape[0]))
        assert got == (sts or (0,) * x.shape[0]), (name, got)


def test_the_returning_node_meets_no_clash():
    x = HR.back_read()
    steps = HR.back_only_steps(x)
    assert steps, "no node re-enters the beam"
    r = HR.report(x)
    assert not any(s["ties"] or s["outside"] for s in r)  # the whole read: the rare block is entered for m_k2 alone


def test_the_crf_twin_meets_ties():
    amb = {name: [SC.want_crf(x[i], init[i], HR.BEAM, -1.0 if "negative" in name else 0.0) for i in range(x.shape[0])]
           for name, x, init in HR.crf_launches()}
    assert all(w[0] == 0 for ws in amb.values() for w in ws)
    assert all(w[3][1] >= 1 for w in amb["crf dyadic"]), "a dyadic CRF read without a tie at ranks 0 / 1 or across the boundary"
    assert amb["crf all equal"][0][3][0] >= 2, "the all-equal CRF read never ties among more than 20 candidates"


@pytest.mark.parametrize("order", ORDERS)
def test_plain_launches_match_the_oracle(fcd, order):
    with tie_order(fcd, order):
        HR.run_plain(fcd)


@pytest.mark.parametrize("order", ORDERS)
def test_crf_twin_matches_the_oracle(fcd, order):
    with tie_order(fcd, order):
        HR.run_crf(fcd)
