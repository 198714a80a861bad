"""The f32 rank count of the headline beam kernels (csrc/device_utils.h, FCD_RANKF4; the guard and the recount in
csrc/beam_wave_step.inc) on the MI355X, where the hardware's v_fma_f32 with clamp is what ranks: the constructed reads of
tests/rank_domain_cases.py against the oracle -- labels, path, out_len and status, exactly, under both tie orders, beams 5
and 3: inside the domain, outside it through every door, on its edges, exact +0 candidates, ties inside it, one half of a
wavefront inside and the other outside, the CRF twin with 4 states, N = 3 and 4.
That the cases enter or avoid the guard as named is established on the CPU: tests/test_rank_domain_emu.py, its twin."""
import pytest

import rank32_cases as RC
import rank_domain_cases as DC
from tie_util import ORDERS, tie_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", DC.BEAMS)
def test_inside_outside_and_halves(fcd, order, beam):
    with tie_order(fcd, order):
        DC.run_all(fcd, beam)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", DC.BEAMS)
def test_crf_and_small_alphabets(fcd, order, beam):
    with tie_order(fcd, order):
        for name, x, init in DC.crf_launches():
            RC.check_crf(fcd, x, init, beam, 0.0, what=name)
        for name, thr, x in DC.small_alphabet_launches():
            RC.check_plain(fcd, x, beam, thr, what=name)
