"""CPU-side check of one time step of the headline beam kernels (csrc/beam_wave_step.inc, the HL forms) on tests/hipemu's
lockstep emulation: the launches of tests/headline_step_cases.py against the oracle -- labels, path, out_len and status,
exactly, under both tie orders, for S = 0 and the CRF twin with 4 states.  The first test establishes from the
reference's own search that every crafted launch reaches the branch it is named after, so that none passes vacuously.
The -m gpu twin is tests/test_gpu_headline_step.py."""
import pytest

import headline_step_cases as HS
from emu_util import emulated_kernels
from tie_util import ORDERS, tie_order


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


def test_the_crafted_cases_reach_what_they_are_named_after():
    for name, thr, x, sts in HS.crafted():
        assert x.shape[0] <= 8 and x.shape[1] <= 40, name
        assert HS.statuses(x, thr) == (sts or (0,) * x.shape[0]), name
        assert HS.reaches(name, thr, x) == "", name


def test_the_random_shapes_are_the_ones_asked_for():
    got = sorted((x.shape[0], x.shape[1]) for _, x in HS.random_launches())
    assert got == sorted((b, t) for t in HS.LENGTHS for b in HS.COUNTS for _ in HS.STYLES)
    assert all(x.shape[2:] == (HS.S, HS.N) and init.shape == (x.shape[0], HS.S) for _, x, init in HS.random_crf_launches())


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
