"""Three forms of the headline beam step (csrc/beam_wave_step.inc, HL -- WSC: the beam width as loop-carried scalar state;
ZSEL: no select where the value is already zero; CHB: the new slot's child entry gathered through bit 0 of the survivor-table
entry) on the MI355X: the reads of tests/headline_width_cases.py against the oracle -- labels, path, out_len and status,
exactly, under both tie orders, beams 1 .. 5, S = 0 and the CRF twin with 4 states.  The launches that share a threshold and
a length travel as one batch.  That the cases reach the situations they are named after is established on the CPU:
tests/test_headline_width_emu.py, its twin."""
import pytest

import headline_width_cases as HW
from tie_util import ORDERS, tie_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("order", ORDERS)
def test_plain_batches_match_the_oracle(fcd, order):
    with tie_order(fcd, order):
        for beam in HW.BEAMS:
            HW.run_plain_batched(fcd, beam)


@pytest.mark.parametrize("order", ORDERS)
def test_crf_twin_batches_match_the_oracle(fcd, order):
    with tie_order(fcd, order):
        for beam in HW.BEAMS:
            HW.run_crf_batched(fcd, beam)
