"""The packed mode of CTC motif detection (ctc_detect_batch_raw(packed=True)) on tests/hipemu's wave64 emulation; see tests/ctc_demux_cases.py.  -m gpu twin: test_gpu_ctc_demux.py."""
import pytest

import ctc_demux_cases as DX
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("name", DX.NAMES)
def test_against_reference(fcd, name):
    DX.run_case(fcd, name)
