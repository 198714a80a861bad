"""-m gpu: CRF motif spotting on torch tensors (fcd_crf_align_dev under fcd_set_crf_spot) and numpy; see tests/crf_spot_cases.py."""
import pytest

import crf_spot_cases as SC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device", ["cuda", None])
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_cases(name, device):
    import fast_ctc_decode_amd as fcd
    SC.run_case(fcd, name, device)
