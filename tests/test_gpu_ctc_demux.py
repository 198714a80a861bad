"""-m gpu: the packed mode of CTC motif detection on torch tensors (fcd_ctc_score_dev under fcd_set_ctc_detect and fcd_set_ctc_detect_packed) and numpy; see tests/ctc_demux_cases.py."""
import pytest

import ctc_demux_cases as DX

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device", ["cuda", None])
@pytest.mark.parametrize("name", DX.NAMES)
def test_cases(name, device):
    import fast_ctc_decode_amd as fcd
    DX.run_case(fcd, name, device)
