"""CTC motif spotting (fcd_ctc_spot_*) on tests/hipemu's wave64 emulation; see tests/ctc_spot_cases.py.  -m gpu twin: test_gpu_ctc_spot.py."""
import pytest

import ctc_spot_cases as SP
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("name", sorted(SP.CASES))
def test_against_reference(fcd, name):
    SP.run_case(fcd, name)


@pytest.mark.parametrize("every_pointer", [False, True])
def test_host_abi(fcd, every_pointer):
    SP.host_abi(fcd, every_pointer)


def test_single_read_function(fcd):
    x = SP.build("across_chunk_K6")["x32"][0]
    seq = "".join("NACGT"[v] for v in SP._M24)
    start, end, logp = fcd.ctc_spot(x, seq, "NACGT")
    assert (start, end) == (50, 73) and fcd.ctc_spot(x, seq, "NACGT", rows=(-90, -50)) == (start, end, logp)
    assert fcd.ctc_spot(x, seq, "NACGT", rows=(0, 20)) is None and fcd.ctc_spot(x, "", "NACGT") is None
