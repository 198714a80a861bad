"""The rank on the 32-bit probability word (csrc/beam_wave_step.inc, R32) on the MI355X: the constructed reads of
tests/rank32_cases.py against the oracle -- labels, path, out_len and status, exactly, under both tie orders, beams 5 and
3: ties at ranks 0 / 1, inside the kept ranks, across the beam boundary and below it, zeros of both signs, subnormals, lone
NaNs, a NaN among several, an empty candidate list, the quicksort handover, one or both halves of a wavefront tied, CRF
with 4 states, f16, ragged lengths, a session fed row by row from device chunks, n-best.
That the cases meet their ties is established on the CPU: tests/test_rank32_emu.py, its twin."""
import numpy as np
import pytest

import rank32_cases as RC
from tie_util import ORDERS, tie_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", RC.BEAMS)
def test_tied_reads(fcd, order, beam):
    with tie_order(fcd, order):
        for name, thr, x in RC.tied_launches():
            assert all(RC.kept_tie_steps(x[i], beam, thr) >= 1 for i in range(x.shape[0])), (name, beam)
            RC.check_plain(fcd, x, beam, thr, what=name)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", RC.BEAMS)
def test_one_half_or_both(fcd, order, beam):
    with tie_order(fcd, order):
        for name, thr, x, tied in RC.half_launches():
            assert tuple(RC.kept_tie_steps(x[i], beam, thr) >= 1 for i in (0, 1)) == tied, (name, beam)
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
    import torch

    with tie_order(fcd, order):
        x, init = RC.crf_launch()
        RC.check_crf(fcd, x, init, beam, 0.0)
        q = RC.tied_launches()[0][2]
        r = fcd.beam_search_batch_raw(torch.from_numpy(q.astype(np.float16)).cuda(), beam, 0.0, True, kernel=RC.SC.KERNEL_WAVE).cpu()
        for i in range(q.shape[0]):
            RC.SC.check_slot(r, i, RC.SC.want_plain(q[i], beam, 0.0, True), "f16 read %d" % i)
        lengths = np.array([RC.T, RC.T - 1, 17, 1, 0, 33], np.int64)
        RC.check_plain(fcd, q, beam, 0.0, lengths=lengths, what="ragged")
        RC.check_plain(fcd, RC.tied_launches()[3][2], beam, 0.0, lengths=np.array([RC.T, 29], np.int64), what="ragged constant")


@pytest.mark.parametrize("order", ORDERS)
def test_session_and_nbest(fcd, order):
    import torch

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()

    with tie_order(fcd, order):
        x = np.stack([RC.quantised(1, 24), RC.constant(24), RC.plain_random(12, 24)])
        RC.run_session(fcd, x, 5, 0.0, to_input=dev, host=False)
        RC.run_session(fcd, x[:2], 3, 0.0, to_input=dev, host=False)
        q = RC.tied_launches()[0][2]
        for beam in RC.BEAMS:
            RC.run_nbest(fcd, q, beam, 0.0, stable=(order == "stable"), lengths=np.array([RC.T, RC.T - 1, 17, 1, 0, 33], np.int64))
            RC.run_nbest(fcd, np.stack([RC.constant(), RC.two_equal(1)]), beam, 0.0, stable=(order == "stable"))
