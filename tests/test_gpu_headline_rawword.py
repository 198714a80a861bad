"""The raw probability table of the headline beam kernels (csrc/beam_wave_step.inc, RAWK: keyed probability words and node
words are formed, and both tables rebuilt, only inside the step's rare block) on the MI355X: the launches of
tests/headline_rawword_cases.py against the oracle -- labels, path, out_len and status, exactly, under both tie orders,
S = 0 and the CRF twin with 4 states.  That the cases reach the branches they are named after is established on the CPU:
tests/test_headline_rawword_emu.py, its twin."""
import pytest

import headline_rawword_cases as HR
from tie_util import ORDERS, tie_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("order", ORDERS)
def test_plain_launches_match_the_oracle(fcd, order):
    with tie_order(fcd, order):
        HR.run_plain(fcd)


@pytest.mark.parametrize("order", ORDERS)
def test_crf_twin_matches_the_oracle(fcd, order):
    with tie_order(fcd, order):
        HR.run_crf(fcd)
