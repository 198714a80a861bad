"""CPU-side check of the CRF transition-probability walk (csrc/crf_transitions.hip, crf_transitions_kernel,
compiled against tests/hipemu's lockstep wave64 emulation) through fcd_crf_transition_probs_host and
crf_transition_probs_batch_raw on numpy, against the float64 restatement tests/crf_transitions_reference.py: the whole table of
tests/crf_transitions_cases.py, the edge cases of the definition, the argument errors at both layers and every limit, the
nullable logz, the single-read function, the composition with the searches, and the launch log.  The -m gpu twin is
tests/test_gpu_crf_transitions.py."""
import ctypes as C

import numpy as np
import pytest

import crf_transitions_cases as TC
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


@pytest.mark.parametrize("case", TC.CASES + [TC.BIG_LDS], ids=[c["name"] for c in TC.CASES + [TC.BIG_LDS]])
def test_against_reference(fcd, case):
    TC.run_case(fcd, case)
    print("%s: err32 %.3g, emulator %.3g" % (case["name"], TC.build_case(case)["err32"], TC.OBSERVED[case["name"]]))


def test_edge_cases(fcd):
    TC.edge_cases(fcd)


def test_argument_errors_and_limits(fcd):
    TC.argument_errors(fcd)


def test_nullable_outputs(fcd):
    TC.nullable_outputs(fcd)


def test_launches_crf_transitions_kernel_only(env):
    fcd, lib = env
    lib.hipemu_launch_log_reset()
    for S, N in ((4, 5), (64, 5), (130, 3)):
        fcd.crf_transition_probs_batch_raw(R.random_scores(np.random.default_rng(S), 5, S, N)[None], layout="dest", out_dtype="float16")
    need = lib.hipemu_launch_log_read(None, 0)
    buf = C.create_string_buffer(need)
    lib.hipemu_launch_log_read(buf, need)
    names = [l for l in buf.value.decode().splitlines() if l]
    assert len(names) == 1 and canonical(names[0]) == "crf_transitions_kernel", names


def test_viterbi_search_finds_the_best_path_of_the_scores(fcd):
    """on peaked scores crf_viterbi_search of (probs, init) is the float64 best path of the SCORES, start state included,
    and its logp + ln init[s0] is that path's score - logZ"""
    rng = np.random.default_rng(8)
    for S, N, T in ((4, 5, 40), (16, 5, 130), (64, 3, 70)):
        x = TC.peaked_scores(rng, 3, T, S, N)
        for out_dtype in ("float32", "float16"):
            r = fcd.crf_transition_probs_batch_raw(x, out_dtype=out_dtype)
            v = fcd.crf_viterbi_search_batch_raw(r.probs, r.init)
            for b in range(3):
                score, s0, rows, labels = TC.best_path64(x[b])
                n = int(v.out_len[b])
                assert int(v.status[b]) == 0 and int(np.argmax(r.init[b])) == s0
                assert v.labels[b, :n].tolist() == labels and v.path[b, :n].tolist() == rows, (S, N, T, out_dtype, b)
                if out_dtype == "float32":
                    assert abs(v.logp[b] + np.log(float(r.init[b, s0])) - (score - r.logz[b])) <= 1e-4 * T


def test_greedy_and_beam_searches_take_the_result(fcd):
    rng = np.random.default_rng(10)
    x = TC.peaked_scores(rng, 1, 60, 16, 5)[0]
    score, s0, rows, labels = TC.best_path64(x)
    want = "".join("NACGT"[l] for l in labels)
    probs, init, logz = fcd.crf_transition_probs(x)
    assert fcd.crf_greedy_search(probs, init, "NACGT")[0] == want
    assert fcd.crf_beam_search(probs, init, "NACGT", 5, 0.0)[0] == want
    for out_dtype in ("float32", "float16"):
        r = fcd.crf_transition_probs_batch_raw(x[None], out_dtype=out_dtype, time_major_out=True)
        g = fcd.crf_greedy_search_batch_raw(r.probs, r.init)
        bm = fcd.crf_beam_search_batch_raw(r.probs, r.init, 5, 0.0)
        n = int(bm.out_len[0])
        assert g.labels[0, :int(g.out_len[0])].tolist() == labels and bm.labels[0, :n].tolist() == labels
        lp = bm.crf_score(r.probs, r.init)
        assert np.isfinite(lp).all() and lp[0, 0] <= 0.0
