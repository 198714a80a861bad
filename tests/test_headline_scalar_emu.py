"""CPU-side check of the wave-uniform predicates of the headline beam kernels (csrc/beam_wave_step.inc, HL: "own candidate
dropped" as a multiple of the kept own-lane bits, the new ids counted with a lane-constant word; and the states in which a
per-half count, width and group mask in scalar registers or an eviction store without the dead-row test would go wrong --
priced and not adopted) on tests/hipemu's lockstep emulation: the launches of tests/headline_scalar_cases.py against the
oracle -- labels, path, out_len and status, exactly, under both tie orders, S = 0 and the CRF twin with 4 states.
The first tests establish, from the reference's own search (headline_scalar_cases.trace), that every crafted read reaches
the state it is named after; a read that does not fails the test.  The emulator poisons device memory and aborts when a
returning node's child row was never stored.
The -m gpu twin is tests/test_gpu_headline_scalar.py."""
import pytest

import headline_scalar_cases as HS
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
    """(launch name, read index, crf) -> trace, computed once"""
    return {(name, i, crf): HS.trace(x[i], thr, crf)
            for name, thr, x, _ in HS.launches() for i in range(x.shape[0]) for crf in MODES}


def widths(tr):
    return [s["width"] for s in tr]


def test_every_launch_is_one_or_two_wavefronts_of_equal_reads(traces):
    for name, thr, x, sts in HS.launches():
        assert 2 <= x.shape[0] <= 4 and 1 <= x.shape[1] <= 130 and x.shape[2] == HS.N, name
        got = tuple(SC.want_plain(x[i], HS.BEAM, thr, True)[0] for i in range(x.shape[0]))
        assert got == (sts or (0,) * x.shape[0]), (name, got)
        xs, init = HS.crf_twin(x)
        got = tuple(SC.want_crf(xs[i], init[i], HS.BEAM, thr)[0] for i in range(x.shape[0]))
        fails = tuple(traces[(name, i, True)][-1]["fail"] for i in range(x.shape[0]))
        assert got == tuple({None: 0, "empty": 1, "nan": 2}[f] for f in fails), (name, got, fails)


def test_the_halves_hold_different_widths(traces):
    narrow = {}
    for crf in MODES:
        met = set()
        for name, full_at in (("widths, narrow below full", 1), ("widths, full below narrow", 0)):
            a, b = widths(traces[(name, 1 - full_at, crf)]), widths(traces[(name, full_at, crf)])
            assert len(a) == len(b) == HS.WIDTH_T
            # the neighbour is full from its first step on; the narrow read holds fewer in some of them
            assert set(b) == {HS.BEAM} and any(w < HS.BEAM for w in a), (name, crf)
            met |= set(a)
            narrow[(name, crf)] = a
        assert met == {1, 2, 3, 4, 5}, (crf, met)
        name = "widths, two narrow halves, two wavefronts"
        for lo, hi in ((0, 1), (2, 3)):
            a, b = widths(traces[(name, lo, crf)]), widths(traces[(name, hi, crf)])
            assert any(u != v and u < HS.BEAM and v < HS.BEAM for u, v in zip(a, b)), (name, lo, crf)
    # plain search: the width shrinks and later grows again, next to a full neighbour (the CRF search adds a candidate per
    # slot in every step: its width never shrinks -- headline_scalar_cases.peaky)
    for name in ("widths, narrow below full", "widths, full below narrow"):
        w = narrow[(name, False)]
        down = [t for t in range(1, len(w)) if w[t] < w[t - 1]]
        assert down and any(w[u] > w[t] for t in down for u in range(t + 1, len(w))), (name, w)
        assert all(w[t] >= w[t - 1] for t in range(1, len(w)) for w in (narrow[(name, True)],)), name


def test_a_half_runs_out_of_beam_while_the_other_runs_on(traces):
    for crf in MODES:
        for name, dead in (("runs out, lower half", 0), ("runs out, upper half", 1)):
            d, o = traces[(name, dead, crf)], traces[(name, 1 - dead, crf)]
            assert d[-1]["fail"] == "empty" and len(d) == 13 and len(o) == 24 and o[-1]["fail"] is None, (name, crf)
        name = "runs out in the last step"
        for i, fails in enumerate((True, False, False, True)):
            tr = traces[(name, i, crf)]
            assert len(tr) == 24 and (tr[-1]["fail"] == "empty") == fails, (name, i, crf)


def test_a_nan_fails_among_several_and_not_alone(traces):
    for crf in MODES:
        name = "NaN among several"
        for i, (at, fails) in enumerate(((6, True), (11, False), (11, False), (11, True))):
            tr = traces[(name, i, crf)]
            assert len(tr) == at + 1 and (tr[-1]["fail"] == "nan") == fails, (name, i, crf)
            if fails:
                assert tr[-1]["n"] >= 2
    for i in (0, 1):  # (plain search: the lone NaN is the first row's only candidate under threshold 0.5)
        tr = traces[("lone NaN", i, False)]
        assert tr[0]["lone_nan"] and tr[0]["n"] == 1 and tr[-1]["fail"] is None and len(tr) == 3, i


def test_a_node_is_evicted_and_re_enters(traces):
    name = "eviction and re-entry"
    for crf in MODES:
        for half in (0, 1):  # a wavefront's lower and upper half
            assert any(any(s["back"] for s in traces[(name, i, crf)]) for i in (half, half + 2)), (crf, half)
        # an evicted node that every new beam entry is at least as deep as: the row the dead-row test skipped
        assert all(any(s["dead"] for s in traces[(name, i, crf)]) for i in range(4)), crf
    assert any(s["back"] for s in traces[(name, 0, False)]) and any(s["back"] for s in traces[(name, 1, True)])


def test_the_eviction_patterns_are_met(traces):
    need = {(True,) * 5, (False,) * 5, (False, False, False, False, True)}
    for crf in MODES:
        for name, i in (("eviction patterns, lower half", 0), ("eviction patterns, upper half", 1)):
            owns = {s["own"] for s in traces[(name, i, crf)] if s["before"] == HS.BEAM}
            assert need <= owns, (name, crf, need - owns)


def test_both_halves_number_more_than_half_a_block_of_new_nodes(traces):
    for crf in MODES:
        a, b = (traces[("new ids in both halves", i, crf)] for i in (0, 1))
        assert any(u["new"] > 16 and v["new"] > 16 for u, v in zip(a, b)), crf  # together more than the step's 32 ids


def test_a_recount_follows_a_width_change(traces):
    for crf in MODES:
        for name, i in (("recount behind a width change, lower half", 0), ("recount behind a width change, upper half", 1)):
            tr = traces[(name, i, crf)]
            assert any(tr[t]["width"] != tr[t]["before"] and tr[t + 1]["recount"] for t in range(len(tr) - 1)), (name, crf)


@pytest.mark.parametrize("order", ORDERS)
def test_plain_launches_match_the_oracle(fcd, order):
    with tie_order(fcd, order):
        HS.run_plain(fcd)


@pytest.mark.parametrize("order", ORDERS)
def test_crf_twin_matches_the_oracle(fcd, order):
    with tie_order(fcd, order):
        HS.run_crf(fcd)
