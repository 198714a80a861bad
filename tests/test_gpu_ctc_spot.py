"""-m gpu: CTC motif spotting on torch tensors (fcd_ctc_align_dev under fcd_set_ctc_spot) and numpy; see tests/ctc_spot_cases.py."""
import pytest

import ctc_spot_cases as SP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("device", ["cuda", None])
@pytest.mark.parametrize("name", sorted(SP.CASES))
def test_cases(fcd, name, device):
    SP.run_case(fcd, name, device)


@pytest.mark.parametrize("every_pointer", [False, True])
def test_host_abi(fcd, every_pointer):
    SP.host_abi(fcd, every_pointer)
