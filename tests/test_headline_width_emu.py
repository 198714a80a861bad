"""CPU-side check of three forms of the headline beam step (csrc/beam_wave_step.inc, HL -- WSC: the beam width as loop-carried
scalar state; ZSEL: no select where the value is already zero; CHB: the new slot's child entry gathered through bit 0 of the
survivor-table entry) on tests/hipemu's lockstep emulation: the launches of tests/headline_width_cases.py against the oracle
-- labels, path, out_len and status, exactly, under both tie orders, beams 1 .. 5, S = 0 and the CRF twin with 4 states.
Under the emulation the step itself checks, in every step of every launch, and aborts with a message: the carried group mask
and widths against the per-lane width formed from the candidate count; the word a slot's own lane received from a push
nobody made; the gathered child entry against the one a look at the source's kind yields.
The first tests establish, from the reference's own search (headline_width_cases.trace), that every crafted read reaches the
situation it is named after; a read that does not fails the test.
The -m gpu twin is tests/test_gpu_headline_width.py."""
import numpy as np
import pytest

import headline_scalar_cases as HS
import headline_width_cases as HW
import session_cases as SC
from emu_util import emulated_kernels
from tie_util import ORDERS, tie_order

MODES = (False, True)  # plain search (S = 0) / the CRF twin (S = 4)


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.fixture(scope="module")
def traces():
    """(launch name, read index, crf) -> trace at beam 5, computed once"""
    return {(name, i, crf): HW.trace(x[i], thr, crf)
            for name, thr, x, _ in HW.launches() for i in range(x.shape[0]) for crf in MODES}


def changes(tr):
    """the steps in which the width changes"""
    return {t for t, s in enumerate(tr) if s["fail"] is None and s["width"] != s["before"]}


def test_every_launch_is_small_and_ends_as_it_says(traces):
    for name, thr, x, sts in HW.launches():
        assert 1 <= x.shape[0] <= 4 and 1 <= x.shape[1] <= 130 and x.shape[2] == HW.N, name
        got = tuple(SC.want_plain(x[i], 5, thr, True)[0] for i in range(x.shape[0]))
        assert got == (sts or (0,) * x.shape[0]), (name, got)
        fails = tuple(traces[(name, i, True)][-1]["fail"] for i in range(x.shape[0]))
        xs, init = HS.crf_twin(x)
        got = tuple(SC.want_crf(xs[i], init[i], 5, thr)[0] for i in range(x.shape[0]))
        assert got == tuple({None: 0, "empty": 1, "nan": 2}[f] for f in fails), (name, got, fails)
    sizes = {x.shape[0] for _, _, x, _ in HW.launches()}
    assert 1 in sizes and 3 in sizes  # a launch of one read; an odd one, whose last wavefront holds one read


def test_the_width_grows_from_one_to_five(traces):
    for crf in MODES:
        for name, n in (("widths grow", 2), ("widths grow, one read", 1)):
            for i in range(n):
                w = HW.widths(traces[(name, i, crf)])
                assert w[0] == 1 and w[-1] == 5 and all(b - a in (0, 1) for a, b in zip(w, w[1:])), (name, i, crf, w)
    # and under a smaller beam it stops there
    x = HW.by_name()["widths grow"][1]
    for beam in HW.BEAMS:
        assert max(HW.widths(HW.trace(x[0], HW.THR_PEAKY, False, beam))) == beam


def test_the_width_shrinks_and_grows_again_mid_read(traces):
    thr, x, _ = HW.by_name()["widths shrink and grow, narrow below full"]
    assert float(np.mean(x[0] < thr)) > 0.5  # the threshold cuts most of the narrow read's rows
    for name, i in (("widths shrink and grow, narrow below full", 0), ("widths shrink and grow, full below narrow", 1)):
        w = HW.widths(traces[(name, i, False)])
        down = [t for t in range(1, len(w)) if w[t] < w[t - 1]]
        assert down and any(w[u] > w[t] for t in down for u in range(t + 1, len(w))), (name, w)


def test_the_halves_differ_and_one_changes_alone(traces):
    for crf in MODES:
        for name, narrow in (("widths shrink and grow, narrow below full", 0), ("widths shrink and grow, full below narrow", 1)):
            a, b = traces[(name, narrow, crf)], traces[(name, 1 - narrow, crf)]
            # the neighbour is full from its first step on: every change of the narrow half is one it makes alone
            assert set(HW.widths(b)) == {5} and len(changes(a) - {0}) >= (1 if crf else 3), (name, crf)
        a, b = (traces[("widths, two narrow halves", i, crf)] for i in (0, 1))
        wa, wb = HW.widths(a), HW.widths(b)
        assert any(u != v and u < 5 and v < 5 for u, v in zip(wa, wb)), crf
        assert changes(a) - changes(b) and changes(b) - changes(a), crf


def test_a_half_runs_out_while_the_other_goes_on(traces):
    for crf in MODES:
        for name, dead in (("runs out, lower half", 0), ("runs out, upper half", 1)):
            d, o = traces[(name, dead, crf)], traces[(name, 1 - dead, crf)]
            assert d[-1]["fail"] == "empty" and len(d) < len(o) and o[-1]["fail"] is None, (name, crf)


def test_a_nan_fails_one_half_in_the_step_that_changes_the_others_width(traces):
    # (plain search: the CRF twin's width never shrinks, and behind its first steps it no longer changes)
    for name, bad in (("NaN beside a width change, lower half", 0), ("NaN beside a width change, upper half", 1)):
        f, o = traces[(name, bad, False)], traces[(name, 1 - bad, False)]
        at = len(f) - 1
        assert f[at]["fail"] == "nan" and f[at]["n"] >= 2 and at in changes(o) and at >= 6, (name, at)
        assert traces[(name, bad, True)][-1]["fail"] == "nan"


def test_the_pushes_and_selects_are_met(traces):
    thr, x, _ = HW.by_name()["zero pushes"]
    assert thr == 0.0 and np.any(x.view(np.uint32) == 0x80000000)  # a -0.0 posterior under threshold 0
    for crf in MODES:
        for i in range(x.shape[0]):
            tr = traces[("zero pushes", i, crf)]
            assert tr[-1]["fail"] is None and len(tr) == x.shape[1]
        assert any(s["zero_push"] for i in range(x.shape[0]) for s in traces[("zero pushes", i, crf)]), crf
        # (the CRF twin alone: with repeats collapsed, the label that reaches a beam entry from its parent is the entry's own tip
        # label, so the extension never passes without the entry's repeat-stay)
        assert not crf or any(s["inc_only"] for name in ("widths, two narrow halves", "source kinds, peaky") for i in (0, 1)
                              for s in traces[(name, i, crf)])
        assert all(any(s["blank_kept"] for s in traces[("source kinds", i, crf)]) for i in (0, 1)), crf


def test_the_three_source_kinds_meet_in_one_step(traces):
    for crf in MODES:
        names = ("source kinds", "source kinds, peaky")
        steps = [s for name in names for i in (0, 1) for s in traces[(name, i, crf)]]
        assert any(s["kinds"] == {"self", "first", "back"} for s in steps), crf
        assert any(s["back_child"] for s in steps), crf


@pytest.mark.parametrize("beam", HW.BEAMS)
@pytest.mark.parametrize("order", ORDERS)
def test_plain_launches_match_the_oracle(fcd, order, beam):
    with tie_order(fcd, order):
        HW.run_plain(fcd, beam)


@pytest.mark.parametrize("beam", HW.BEAMS)
@pytest.mark.parametrize("order", ORDERS)
def test_crf_twin_matches_the_oracle(fcd, order, beam):
    with tie_order(fcd, order):
        HW.run_crf(fcd, beam)
