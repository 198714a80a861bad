"""-m gpu: the twin of tests/test_crf_edits_tiers_emu.py -- one small crf_edits call on device tensors for every
instantiation of crfp_back_kernel, checked against the restatements."""
import pytest

import crf_edits_cases as EC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("tier", EC.TIERS, ids=["k%d_m%d_n%d" % t for t in EC.TIERS])
def test_tier(fcd, tier):
    EC.tier_check(*EC.tier_call(fcd, tier, device="cuda"), tier)
