"""CPU-side check of the divisions at the source lanes (csrc/beam_wave_step.inc, DSRC) on tests/hipemu's lockstep emulation:
the constructed reads of tests/divide_source_cases.py against the oracle, T in {1, 2, 7, 65}, 1 and 3 reads, beams 1 .. 5,
both tie orders, f16, ragged lengths, the counting instantiations, CRF with 4 states, and sessions pushed row by row.
The -m gpu twin is tests/test_gpu_divide_source.py."""
import numpy as np
import pytest

import divide_source_cases as DC
import session_cases as SC
from emu_util import emulated_kernels
from tie_util import ORDERS, tie_order


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


def test_the_oracle_accepts_every_constructed_read():
    """no input is malformed: the oracle returns a status for each, and the cases are what they claim to be"""
    for T in DC.TS:
        for thr in DC.THRS:
            for x in DC.group(thr, T):
                st = SC.want_plain(x, 5, thr, True)[0]
                assert st in (0, 1, 2), (T, thr, st)
        x, init = DC.crf_group(0.0, T)
        for i in range(3):
            assert SC.want_crf(x[i], init[i], 5, 0.0)[0] in (0, 1, 2), (T, i)
    # (c): the all-zero read divides 0 by 0 in its first step and meets the NaNs in its second
    assert SC.want_plain(DC.zeros(1), 5, 0.0, True)[0] == 0
    assert SC.want_plain(DC.zeros(2), 5, 0.0, True)[0] == 2
    # (d): the lone NaN candidate is not compared: the first step succeeds
    assert SC.want_plain(DC.lone_nan(1), 5, 0.5, True)[0] == 0
    # (f): steps that settle twice exist from beam 5 / T 7 on
    assert DC.tied_steps(7, 5) > 0 and DC.tied_steps(65, 5) > 0


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
    with tie_order(fcd, order):
        for thr in DC.THRS:
            DC.run_session(fcd, thr, 7, 5)
