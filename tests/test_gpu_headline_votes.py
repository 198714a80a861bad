"""The wave-wide votes of the headline beam kernels (csrc/beam_wave_step.inc, the HL family: lane predicates formed as masks,
votes on bare compares joined in scalar registers) on the MI355X: the constructed reads of tests/headline_votes_cases.py
against the oracle -- labels, path, out_len and status, exactly, under both tie orders, beams 5 and 3, over N = 3, 4, 5
and the CRF twin with 4 states.  Launches of 1 .. 8 reads, T <= 48.
That the reads reach the states they are named after is established on the CPU: tests/test_headline_votes_emu.py, its twin."""
import pytest

import headline_votes_cases as HV
from tie_util import ORDERS, tie_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", HV.BEAMS)
def test_plain(fcd, order, beam):
    with tie_order(fcd, order):
        HV.run_plain(fcd, beam)


@pytest.mark.parametrize("n", (3, 4))
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", HV.BEAMS)
def test_small_alphabets(fcd, order, beam, n):
    with tie_order(fcd, order):
        HV.run_small(fcd, beam, n)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("beam", HV.BEAMS)
def test_crf_twin(fcd, order, beam):
    with tie_order(fcd, order):
        HV.run_crf(fcd, beam)
