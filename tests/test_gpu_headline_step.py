"""One time step of the headline beam kernels (csrc/beam_wave_step.inc, the HL forms) on the MI355X: the launches of
tests/headline_step_cases.py against the oracle -- labels, path, out_len and status, exactly, under both tie orders, for
S = 0 and the CRF twin with 4 states.  That the crafted launches reach the branches they are named after is established
on the CPU: tests/test_headline_step_emu.py, its twin."""
import pytest

import headline_step_cases as HS
from tie_util import ORDERS, tie_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("order", ORDERS)
def test_random_reads_match_the_oracle(fcd, order):
    with tie_order(fcd, order):
        HS.run_random(fcd)


@pytest.mark.parametrize("order", ORDERS)
def test_random_crf_reads_match_the_oracle(fcd, order):
    with tie_order(fcd, order):
        HS.run_random_crf(fcd)


@pytest.mark.parametrize("order", ORDERS)
def test_crafted_reads_match_the_oracle(fcd, order):
    with tie_order(fcd, order):
        HS.run_crafted(fcd)
