"""CPU-side check of the CRF edge marginals (csrc/crf_transitions.hip, crf_marginals_kernel: crf_transitions_walk, then
crf_marginals_forward; compiled against tests/hipemu's lockstep wave64 emulation) through fcd_crf_marginals_host and
crf_marginals_batch_raw on numpy, against the float64 restatement tests/crf_marginals_reference.py: the whole table of
tests/crf_marginals_cases.py, the edge cases of the definition, the argument errors at both layers and every limit, the
nullable emit and logz, untouched rows and spare elements, the agreement with crf_transition_probs, and the launch log.
The -m gpu twin is tests/test_gpu_crf_marginals.py."""
import ctypes as C

import numpy as np
import pytest

import crf_marginals_cases as MC
import crf_transitions_reference as R
from emu_util import emulated_kernels
from instantiation_cases import canonical


@pytest.fixture(scope="module")
def env():
    import fast_ctc_decode_amd as m
    with emulated_kernels() as lib:
        lib.hipemu_launch_log_read.restype = C.c_size_t
        lib.hipemu_launch_log_read.argtypes = [C.c_char_p, C.c_size_t]
        yield m, lib


@pytest.fixture(scope="module")
def fcd(env):
    return env[0]


@pytest.mark.parametrize("case", MC.CASES + [MC.BIG_LDS], ids=[c["name"] for c in MC.CASES + [MC.BIG_LDS]])
def test_against_reference(fcd, case):
    MC.run_case(fcd, case)
    print("%s: err32 %.3g, emulator %.3g" % (case["name"], MC.build_case(case)["merr32"], MC.OBSERVED[case["name"]]))


def test_edge_cases(fcd):
    MC.edge_cases(fcd)


def test_argument_errors_and_limits(fcd):
    MC.argument_errors(fcd)


def test_nullable_outputs_and_untouched_elements(fcd):
    MC.nullable_outputs(fcd)


def test_launches_crf_marginals_kernel_only(env):
    fcd, lib = env
    lib.hipemu_launch_log_reset()
    for S, N in ((4, 5), (64, 5), (130, 3)):
        fcd.crf_marginals_batch_raw(R.random_scores(np.random.default_rng(S), 5, S, N)[None], layout="dest")
    need = lib.hipemu_launch_log_read(None, 0)
    buf = C.create_string_buffer(need)
    lib.hipemu_launch_log_read(buf, need)
    names = [l for l in buf.value.decode().splitlines() if l]
    assert len(names) == 1 and canonical(names[0]) == "crf_marginals_kernel", names
