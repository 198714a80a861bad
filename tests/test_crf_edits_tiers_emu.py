"""CPU-side, on tests/hipemu's emulator: one small crf_edits call for every (states per lane, chain slots, labels)
instantiation of crfp_back_kernel -- every one carries the insertion and the deletion walk (include/fcd.h: the limits are
crf_posterior's, tier for tier, so no call is refused for registers) -- at the smallest shape that selects it: stride = T,
exact mode, T = 40 / 64 / 128 / 256 for 1 / 2 / 4 / 8 states per lane (128 for 3).  The launch log of the call holds exactly
crfp_fwd_kernel<K> and crfp_back_kernel<K,MM,NB>, and the result is the restatements'.  The -m gpu twin is
tests/test_gpu_crf_edits_tiers.py."""
import ctypes as C

import pytest

import crf_edits_cases as EC
import instantiation_cases as IC
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels() as lib:
        lib.hipemu_launch_log_read.restype = C.c_size_t
        lib.hipemu_launch_log_read.argtypes = [C.c_char_p, C.c_size_t]
        yield m, lib


def launched(lib):
    need = lib.hipemu_launch_log_read(None, 0)
    buf = C.create_string_buffer(need)
    assert lib.hipemu_launch_log_read(buf, need) == need
    return {IC.canonical(l) for l in buf.value.decode().splitlines() if l}


@pytest.mark.parametrize("tier", EC.TIERS, ids=["k%d_m%d_n%d" % t for t in EC.TIERS])
def test_tier(fcd, tier):
    m, lib = fcd
    lib.hipemu_launch_log_reset()
    out = EC.tier_call(m, tier)
    names = launched(lib)
    lib.hipemu_launch_log_reset()
    assert names == {"crfp_fwd_kernel<%d>" % tier[0], "crfp_back_kernel<%d,%d,%d>" % tier}, names
    EC.tier_check(*out, tier)


def test_the_tiers_are_the_budget_tests():
    import test_crf_posterior_budget as B
    assert sorted(EC.TIERS) == sorted(B.TIERS)
