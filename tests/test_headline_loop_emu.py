"""CPU-side check of the loop-carried forms of the headline beam kernels (csrc/beam_wave.hip, csrc/beam_wave_step.inc, the HL
family) on tests/hipemu's lockstep emulation: the launches of tests/headline_loop_cases.py against the oracle -- labels,
path, out_len and status, exactly, under both tie orders.  The refill address of the row FIFO (every length around the six
rows of a register and the 42 rows in flight, contiguous and on padded views, S = 0 and the S = 4 twin), the per-half
candidate counts (two unlike reads in one wavefront, beams 1 .. 5, collapse on and off, thresholds 0 and 0.1) and the
divisor (a top probability of 0, -0.0, denormals, ranks 0 and 1 tied among more than 20 candidates).
The first test establishes, from the reference's own search, that the crafted launches reach the cases they are named after;
it needs no product code."""
import numpy as np
import pytest

import headline_loop_cases as HL
from emu_util import emulated_kernels
from tie_util import ORDERS, tie_order


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


def test_the_launches_reach_the_cases_they_are_named_after():
    for beam in HL.BEAMS:
        for collapse in (True, False):
            for thr in HL.THRS:
                for name, x in HL.half_launches():
                    assert HL.half_reaches(name, x, beam, thr, collapse) == "", (name, beam, thr, collapse)
    for name, thr, x in HL.divisor_launches():
        assert HL.divisor_reaches(name, thr, x) == "", name
    # the padded view: the same values, no stride the contiguous array has
    x = HL.refill_launches()[-1][1]
    v = HL.padded_view(x)
    assert np.array_equal(v, x) and v.strides[2] == 8 and v.strides[1] > 8 * HL.N and v.strides[0] > v.strides[1] * x.shape[1]
    assert sorted({xx.shape[1] for _, xx in HL.refill_launches()}) == sorted(HL.REFILL_LENGTHS)
    assert all(xx.shape[0] <= 8 and xx.shape[1] <= 130 for xx in HL.all_launches())
    assert [HL.small_lengths(n)[2] * n <= 32 < (HL.small_lengths(n)[2] + 1) * n for n in (3, 4)] == [True, True]


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
