"""The divisions at the source lanes (csrc/beam_wave_step.inc, DSRC) on the MI355X: the constructed reads of
tests/divide_source_cases.py against the oracle -- IEEE division of subnormals, 0 / 0, a NaN divisor, a child candidate on
top, steps that settle twice -- for T in {1, 2, 7, 65}, 1 and 3 reads, beams 1 .. 5, both tie orders, f16, ragged lengths,
the counting instantiations, CRF with 4 states, and sessions pushed row by row from device chunks.
The CPU twin is tests/test_divide_source_emu.py."""
import numpy as np
import pytest

import divide_source_cases as DC
from tie_util import ORDERS, tie_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("T", DC.TS)
def test_constructed_reads(fcd, order, T):
    with tie_order(fcd, order):
        for beam in DC.BEAMS:
            DC.run_shapes(fcd, T, beam)


@pytest.mark.parametrize("T", (2, 7))
def test_f16_ragged_counted(fcd, T):
    with tie_order(fcd, "pdq178"):
        DC.run_variants(fcd, T, 5)
        DC.run_variants(fcd, T, 3)


@pytest.mark.parametrize("order", ORDERS)
def test_session_row_by_row(fcd, order):
    import torch

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()

    with tie_order(fcd, order):
        for thr in DC.THRS:
            DC.run_session(fcd, thr, 7, 5, to_input=dev, host=False)
