"""CPU-side check of the rank on the 32-bit probability word (csrc/beam_wave_step.inc, R32) on tests/hipemu's lockstep
emulation: the constructed reads of tests/rank32_cases.py against the oracle -- labels, path, out_len and status, exactly,
under both tie orders, beams 5 and 3.  Ties at ranks 0 / 1, inside the kept ranks, across the beam boundary and wholly below
it; many-way ties at +0.0 / -0.0; subnormals; lone NaNs (the all-ones negative one included); a NaN among several; an
empty candidate list; more than 20 candidates with a kept tie (the quicksort handover); both halves of a wavefront tied
and only one; CRF with 4 states; f16; ragged lengths; a session fed row by row; n-best.
The first test establishes, from the reference's own search, that the tied cases meet the ties they are named after.
The -m gpu twin is tests/test_gpu_rank32.py."""
import numpy as np
import pytest

import rank32_cases as RC
import session_cases as SC
from emu_util import emulated_kernels
from tie_util import ORDERS, tie_order


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


def test_the_cases_meet_the_ties_they_are_named_after():
    for beam in RC.BEAMS:
        met = set()
        alone_below = False
        for name, thr, x in RC.tied_launches():
            for i in range(x.shape[0]):
                assert RC.kept_tie_steps(x[i], beam, thr) >= 1, (name, beam, i)
                prof = RC.tie_profile(x[i], beam, thr)
                met |= set().union(*prof)
                alone_below = alone_below or any(s == {"below"} for s in prof)
            # every read of the launch: the oracle's own counter of ties at ranks 0 / 1 or across the boundary
            assert all(RC.counted(x[i], beam, thr)[1] >= 1 for i in range(x.shape[0])), (name, beam)
        assert met >= set(RC.CLASSES), (beam, met)
        assert alone_below, beam  # a step whose only tie lies wholly below the boundary: the branch must stay out of it
        if beam == 5:  # more than 20 candidates with a kept tie: the quicksort's order (the oracle's first counter)
            assert "many" in met
            assert RC.counted(RC.constant(), 5, 0.0)[0] >= 1 and RC.counted(RC.quantised(1), 5, 0.0)[0] >= 1
        for name, thr, x, tied in RC.half_launches():
            for i in (0, 1):
                n = RC.kept_tie_steps(x[i], beam, thr)
                assert (n >= 1) == tied[i], (name, beam, i, n)
                if not tied[i]:
                    assert RC.classes_met(x[i], beam, thr) == set(), (name, beam, i)  # no two candidates ever equal
        x, init = RC.crf_launch()
        for i in range(x.shape[0]):
            assert SC.want_crf(x[i], init[i], beam, 0.0)[3][1] >= 1, (beam, i)
    # zero columns: the tied candidates are zeros of both signs
    z = RC.zero_cols(1)
    assert (z[:, 2:] == 0).all() and np.signbit(z[:, 2:]).any() and not np.signbit(z[:, 2:]).all()
    for name, thr, x, sts in RC.failing_launches():
        for beam in RC.BEAMS:
            got = tuple(SC.want_plain(x[i], beam, thr, True)[0] for i in range(x.shape[0]))
            assert got == (sts or (0,) * x.shape[0]), (name, beam, got)
    # the lone NaN of the second read has probability word 0: !(NaN < thr) passes, its key is the node word alone
    assert RC.lone_nan(0xFFFFFFFF)[0, 1].view(np.uint32) == 0xFFFFFFFF


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", RC.BEAMS)
def test_tied_reads(fcd, order, beam):
    with tie_order(fcd, order):
        for name, thr, x in RC.tied_launches():
            RC.check_plain(fcd, x, beam, thr, what=name)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", RC.BEAMS)
def test_one_half_or_both(fcd, order, beam):
    with tie_order(fcd, order):
        for name, thr, x, _ in RC.half_launches():
            RC.check_plain(fcd, x, beam, thr, what=name)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", RC.BEAMS)
def test_nan_and_empty(fcd, order, beam):
    with tie_order(fcd, order):
        for name, thr, x, _ in RC.failing_launches():
            RC.check_plain(fcd, x, beam, thr, what=name)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", RC.BEAMS)
def test_crf_f16_ragged(fcd, order, beam):
    with tie_order(fcd, order):
        x, init = RC.crf_launch()
        RC.check_crf(fcd, x, init, beam, 0.0)
        q = RC.tied_launches()[0][2]
        RC.check_plain(fcd, q.astype(np.float16), beam, 0.0, what="f16")  # (k / 4: exact in binary16)
        lengths = np.array([RC.T, RC.T - 1, 17, 1, 0, 33], np.int64)
        RC.check_plain(fcd, q, beam, 0.0, lengths=lengths, what="ragged")
        RC.check_plain(fcd, RC.tied_launches()[3][2], beam, 0.0, lengths=np.array([RC.T, 29], np.int64), what="ragged constant")


@pytest.mark.parametrize("order", ORDERS)
def test_session_and_nbest(fcd, order):
    with tie_order(fcd, order):
        x = np.stack([RC.quantised(1, 24), RC.constant(24), RC.plain_random(12, 24)])
        RC.run_session(fcd, x, 5, 0.0)
        RC.run_session(fcd, x[:2], 3, 0.0)
        q = RC.tied_launches()[0][2]
        for beam in RC.BEAMS:
            RC.run_nbest(fcd, q, beam, 0.0, stable=(order == "stable"), lengths=np.array([RC.T, RC.T - 1, 17, 1, 0, 33], np.int64))
            RC.run_nbest(fcd, np.stack([RC.constant(), RC.two_equal(1)]), beam, 0.0, stable=(order == "stable"))
