"""CRF motif spotting (fcd_crf_spot_*) on tests/hipemu's wave64 emulation; see tests/crf_spot_cases.py.  -m gpu twin: test_gpu_crf_spot.py."""
import pytest

import crf_spot_cases as SC
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_against_reference(fcd, name):
    SC.run_case(fcd, name)
