"""The wave-uniform predicates of the headline beam kernels (csrc/beam_wave_step.inc, HL: "own candidate dropped" as a
multiple of the kept own-lane bits in scalar registers; beam widths that differ between the halves, a half that runs out, the
numbering of the upper half's new nodes) on the MI355X: the launches of tests/headline_scalar_cases.py against the
oracle -- labels, path, out_len and status, exactly, under both tie orders, S = 0 and the CRF twin with 4 states.  That the
cases reach the states they are named after is established on the CPU: tests/test_headline_scalar_emu.py, its twin."""
import pytest

import headline_scalar_cases as HS
from tie_util import ORDERS, tie_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("order", ORDERS)
def test_plain_launches_match_the_oracle(fcd, order):
    with tie_order(fcd, order):
        HS.run_plain(fcd)


@pytest.mark.parametrize("order", ORDERS)
def test_crf_twin_matches_the_oracle(fcd, order):
    with tie_order(fcd, order):
        HS.run_crf(fcd)
