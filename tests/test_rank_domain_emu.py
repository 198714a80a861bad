"""CPU-side check of the f32 rank count of the headline beam kernels (csrc/device_utils.h, FCD_RANKF4; the guard and the
recount in csrc/beam_wave_step.inc) on tests/hipemu's lockstep emulation: the constructed reads of
tests/rank_domain_cases.py against the oracle -- labels, path, out_len and status, exactly, under both tie orders, beams 5
and 3.  Reads that stay inside the domain of the count on every step, reads that leave it through each door (tiny and
subnormal, huge and infinite, negative and -0.0, NaNs, one ulp past either edge), alone and mixed with in-domain candidates
of the same half, candidates exactly on the edges, exact +0 candidates, ties inside the domain (the clash branch and the
quicksort hand-over behind it), one half of a wavefront inside and the other outside, the CRF twin with 4 states, N = 3
and 4.
The first test establishes, from the reference's own search, that each case enters or avoids the guard as it is named.
The emulator's clamp is the plain-C++ twin of the instruction's; the hardware's is checked by tests/test_gpu_rank_domain.py."""
import numpy as np
import pytest

import rank32_cases as RC
import rank_domain_cases as DC
from emu_util import emulated_kernels
from tie_util import ORDERS, tie_order


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


def test_the_cases_enter_or_avoid_the_guard_as_named():
    f = np.float32
    assert DC.in_domain(0.0) and DC.in_domain(-0.0) and DC.in_domain(DC.P_LO) and DC.in_domain(DC.P_HI)
    assert not DC.in_domain(np.nextafter(DC.P_LO, f(0))) and not DC.in_domain(np.nextafter(DC.P_HI, f(np.inf)))
    assert not DC.in_domain(f(-0.25)) and not DC.in_domain(f(np.nan)) and not DC.in_domain(f(np.inf))
    assert not DC.in_domain(f(2.0 ** -149))
    for beam in DC.BEAMS:
        for name, thr, x in DC.inside_launches():
            for i in range(x.shape[0]):
                assert not any(DC.outside_steps(x[i], beam, thr)), (name, beam, i)
        for name, thr, x, first in DC.outside_launches():
            for i in range(x.shape[0]):
                st = DC.outside_steps(x[i], beam, thr)
                assert any(st), (name, beam, i)
                assert not first or st[0], (name, beam, i)
        for name, thr, x in DC.edge_launches():
            for i in range(x.shape[0]):
                assert not DC.outside_steps(x[i], beam, thr)[0], (name, beam, i)
        for name, thr, x, out in DC.half_launches():
            assert tuple(any(DC.outside_steps(x[i], beam, thr)) for i in (0, 1)) == out, (name, beam)
        # the tied cases inside the domain still meet kept ties: the clash branch fires without the guard
        for name, thr, x in DC.inside_launches()[2:5]:
            assert all(RC.kept_tie_steps(x[i], beam, thr) >= 1 for i in range(x.shape[0])), (name, beam)
        # exact +0 candidates exist in the case named after them (and are inside)
        z = DC.plus_zero(41)
        assert (z[:, 3:] == 0).all() and not np.signbit(z[:, 3:]).any()
    # mixed with in-domain candidates of the same half, on the first step already
    for name, thr, x, _ in DC.outside_launches():
        if name in ("one column 2^-80", "one column 2^40") or name.startswith("one ulp"):
            assert all(DC.mixed_steps(x[i], 5, thr) for i in range(x.shape[0])), name
    # the doors of rank32_cases.failing_launches(): the lone NaNs and the NaN among several are outside
    for name, thr, x, _ in RC.failing_launches()[:2]:
        assert any(DC.outside_steps(x[0], 5, thr)), name


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
