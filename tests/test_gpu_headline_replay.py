"""The rare block of the headline beam kernels (csrc/beam_wave_step.inc, RSORT: the quicksort of a tie-flagged step
replayed in registers, part of the step parked in LDS around it) on the MI355X: the launches of
tests/headline_replay_cases.py against the oracle -- labels, path, out_len and status, exactly, under both tie orders.
That the cases meet what they are named after is established on the CPU: tests/test_headline_replay_emu.py, its twin."""
import pytest

import headline_replay_cases as HC
import rank32_cases as RC
from tie_util import ORDERS, tie_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


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
