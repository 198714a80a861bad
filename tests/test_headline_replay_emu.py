"""CPU-side check of the rare block of the headline beam kernels (csrc/beam_wave_step.inc, RSORT: the quicksort of a
tie-flagged step replayed in registers, fifteen words per lane parked in LDS around it) on tests/hipemu's lockstep
emulation: the launches of tests/headline_replay_cases.py against the oracle -- labels, path, out_len and status,
exactly, under both tie orders.  The first test establishes from the reference's own search that the cases meet what
they are named after.  The -m gpu twin is tests/test_gpu_headline_replay.py."""
import numpy as np
import pytest

import headline_replay_cases as HC
import rank32_cases as RC
import session_cases as SC
from emu_util import emulated_kernels
from tie_util import ORDERS, tie_order


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


def test_the_cases_meet_what_they_are_named_after():
    c = RC.constant(HC.T)
    many = HC.many_tie_steps(c, 0.0)
    assert len(many) >= HC.T // 2 and many[0] == 2 and many[-1] == HC.T - 1, many  # from the third row to the last one
    counts = [n for _, _, n in HC.profile(c, HC.BEAM, 0.0)]
    assert all(counts[t] > 20 for t in many) and max(counts) <= 25
    assert RC.tie_profile(c, HC.BEAM, 0.0)[0] != set()  # the first row: five equal candidates (the recount)
    assert RC.counted(c, HC.BEAM, 0.0)[0] >= len(many)  # the oracle's own counter of kept ties above 20 candidates
    assert RC.classes_met(RC.plain_random(12, HC.T), HC.BEAM, 0.0) == set()  # the half that must not be flagged
    for name, thr, x, sts in HC.launches():
        assert x.shape[0] <= 8 and x.shape[1] <= 64, name
        got = tuple(SC.want_plain(x[i], HC.BEAM, thr, True)[0] for i in range(x.shape[0]))
        assert got == (sts or (0,) * x.shape[0]), (name, got)
        # every launch has a half that is flagged in a step in which its wavefront's other half still runs
        assert any(HC.many_tie_steps(x[i], thr) for i in range(x.shape[0])), name
    # the step in which the neighbour fails / meets its NaN is a flagged one for the all-equal read
    t0 = HC.T0
    assert t0 in HC.many_tie_steps(c, 0.05) and t0 in many and {3, t0} <= set(HC.many_tie_steps(c, 0.15)) and HC.T - 1 in many
    assert len(HC.profile(HC.failing_row(t0), HC.BEAM, 0.05)) == t0 and len(HC.profile(HC.nan_row(t0), HC.BEAM, 0.0)) == t0
    for first in (t0, 3):
        lone = HC.profile(HC.lone_nan_read(first), HC.BEAM, 0.15)
        assert len(lone) == HC.T and all(n == 1 for _, _, n in lone[first:])
    # a node comes back into the beam at a step in which the all-equal read of the same wavefront is flagged
    back = [t for t, (_, re, _) in enumerate(HC.profile(HC.reentering(), HC.BEAM, 0.0)) if re]
    assert set(back) & set(HC.many_tie_steps(RC.constant(64), 0.0)), back
    x, init = HC.crf_launch()
    assert HC.counted_crf(x[0], init[0])[0] >= 1, "the CRF twin never ties among more than 20 candidates"


@pytest.mark.parametrize("order", ORDERS)
def test_launches_match_the_oracle(fcd, order):
    with tie_order(fcd, order):
        for name, thr, x, _ in HC.launches():
            RC.check_plain(fcd, x, HC.BEAM, thr, what=name)


@pytest.mark.parametrize("order", ORDERS)
def test_crf_twin_matches_the_oracle(fcd, order):
    with tie_order(fcd, order):
        x, init = HC.crf_launch()
        RC.check_crf(fcd, x, init, HC.BEAM, 0.0, what="crf all equal")
