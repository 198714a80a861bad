"""-m gpu: CRF motif occurrence posteriors on torch tensors (fcd_crf_score_dev under fcd_set_crf_detect) and numpy; see tests/crf_detect_cases.py."""
import pytest

import crf_detect_cases as DC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device", ["cuda", None])
@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_cases(name, device):
    import fast_ctc_decode_amd as fcd
    DC.run_case(fcd, name, device)
