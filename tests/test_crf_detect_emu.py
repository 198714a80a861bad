"""CRF motif occurrence posteriors (fcd_crf_detect_*) on tests/hipemu's wave64 emulation; see tests/crf_detect_cases.py.  -m gpu twin: test_gpu_crf_detect.py."""
import pytest

import crf_detect_cases as DC
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_against_reference(fcd, name):
    DC.run_case(fcd, name)
