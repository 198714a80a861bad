"""The loop-carried forms of the headline beam kernels (csrc/beam_wave.hip, csrc/beam_wave_step.inc, the HL family) on the
MI355X: the launches of tests/headline_loop_cases.py against the oracle -- labels, path, out_len and status, exactly, under
both tie orders.  At most 8 reads of at most 130 rows per launch.
That the crafted launches reach the cases they are named after is established on the CPU: tests/test_headline_loop_emu.py,
its twin."""
import pytest

import headline_loop_cases as HL
from tie_util import ORDERS, tie_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("view", (False, True), ids=("contiguous", "view"))
@pytest.mark.parametrize("order", ORDERS)
def test_refill(fcd, order, view):
    with tie_order(fcd, order):
        HL.run_refill(fcd, view)


@pytest.mark.parametrize("view", (False, True), ids=("contiguous", "view"))
@pytest.mark.parametrize("n", (3, 4))
@pytest.mark.parametrize("order", ORDERS)
def test_refill_small_alphabets(fcd, order, n, view):
    with tie_order(fcd, order):
        HL.run_refill_small(fcd, n, view)


@pytest.mark.parametrize("view", (False, True), ids=("contiguous", "view"))
@pytest.mark.parametrize("order", ORDERS)
def test_refill_crf_twin(fcd, order, view):
    with tie_order(fcd, order):
        HL.run_refill_crf(fcd, view)


@pytest.mark.parametrize("collapse", (True, False), ids=("collapse", "no-collapse"))
@pytest.mark.parametrize("beam", HL.BEAMS)
@pytest.mark.parametrize("order", ORDERS)
def test_per_half_counts(fcd, order, beam, collapse):
    with tie_order(fcd, order):
        HL.run_halves(fcd, beam, collapse)


@pytest.mark.parametrize("order", ORDERS)
def test_divisor(fcd, order):
    with tie_order(fcd, order):
        HL.run_divisor(fcd)
