"""Far-offset cases of fcd_crf_occupancy_dev and fcd_crf_score_dev with the handle's wide switch on
(fcd_set_crf_lattice_wide), on the emulator: the builders and checkers of tests/far_offset_cases.py (lattice_far_case with
kind "crf", family "occupancy", whose logp is held to the score family's bits on the same case) on the table's own handle.
T = 520, exact lattice, y.stride = T: 521 states, so every call here runs the LDS-resident walks (the launch log holds it to
crfp_fwd_kernel<8> and crfp_back_kernel<8, 2, 4>) -- with the occupancy blocks 2^31 + 4 floats apart (written and
accumulated), the reads 2^31 + 16 elements apart, and the labellings 2^32 + 4 labels apart.  Far == compact bit for bit,
compact against the float64 restatement (tests/crf_occupancy_cases.py's checker), and a workspace that does not grow with
a stride."""
import contextlib
import ctypes as C

import pytest

import far_offset_cases as F
import instantiation_cases as IC
from emu_util import emulated_kernels

T = 520


@pytest.fixture(scope="module")
def env():
    with emulated_kernels() as lib:
        lib.hipemu_launch_log_read.restype = C.c_size_t
        lib.hipemu_launch_log_read.argtypes = [C.c_char_p, C.c_size_t]
        e = F.Env()
        e.emu = lib
        yield e
        e.close()


@contextlib.contextmanager
def wide(env):
    env.h.set_crf_lattice_wide(True)
    try:
        yield
    finally:
        env.h.set_crf_lattice_wide(False)


def launched(env):
    need = env.emu.hipemu_launch_log_read(None, 0)
    buf = C.create_string_buffer(need)
    assert env.emu.hipemu_launch_log_read(buf, need) == need
    env.emu.hipemu_launch_log_reset()
    return {IC.canonical(l) for l in buf.value.decode().splitlines() if l}


def _run(env, **far):
    seen = []

    def look():
        got = launched(env)
        seen.append(got)
        return got
    launched(env)  # (what ran before this case is not its business)
    with wide(env):
        F.lattice_far_case(env, "crf", "occupancy", 0, 2, 1, T=T, launched=look, **far)
    # (look 0: the score family's call on the case, and the search that made its labellings; 1: the compact call, 2: the far call)
    assert {n for n in seen[0] if n.startswith(("crfp_", "crf_lattice_"))} == {"crfp_fwd_kernel<8>"}, seen[0]
    for got in seen[1:]:
        assert {n for n in got if n.startswith(("crfp_", "crf_lattice_"))} == {"crfp_fwd_kernel<8>", "crfp_back_kernel<8,2,4>"}, got


@pytest.mark.parametrize("accumulate", [0, 1])
def test_far_blocks(env, accumulate):
    _run(env, occ=F.OccLayout(stride_row=F.OCC_FAR_ROW, accumulate=accumulate))


def test_far_reads(env):
    _run(env, layout=F.Layout(stride_read=2 ** 31 + 16), dtype="f16")


def test_far_labellings(env):
    _run(env, y_stride=2 ** 32 + 4)
