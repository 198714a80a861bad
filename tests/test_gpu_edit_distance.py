"""-m gpu: batched edit distance on torch tensors (fcd_duplex_envelope_dev under fcd_set_edit_distance) and numpy; see tests/edit_distance_cases.py."""
import pytest

import edit_distance_cases as EC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device", ["cuda", None])
@pytest.mark.parametrize("name", sorted(EC.CASES))
def test_cases(name, device):
    import fast_ctc_decode_amd as fcd
    EC.run_case(fcd, name, device)
