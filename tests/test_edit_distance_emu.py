"""Batched edit distance (fcd_edit_distance_host) on tests/hipemu's wave64 emulation; see tests/edit_distance_cases.py.  -m gpu twin: test_gpu_edit_distance.py."""
import pytest

import edit_distance_cases as EC
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("name", sorted(EC.CASES))
def test_against_reference(fcd, name):
    EC.run_case(fcd, name)
