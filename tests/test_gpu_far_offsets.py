"""GPU twin of tests/test_far_offsets_emu.py: every entry point of the C ABI on device buffers whose element offsets pass
2^31 and whose byte offsets pass 2^32 (tests/far_offset_cases.py: the table, the builders and the checkers) -- where the
kernels' 32-bit address tricks (byte-offset slabs, wave-uniform bases with one vector offset) actually run.

Memory: ONE pool of 8.75 GiB, made once with torch.empty and never filled or copied as a whole; every case carves its arrays
from it and writes / reads back only the rows it touches.  The arena tests swap it for a pool of 1 GiB (whichever order the
tests run in, the pool is the size the test at hand wants) and hold at most 12 GiB, arena included."""
import ctypes as C
import time

import numpy as np
import pytest

import far_offset_cases as F

pytestmark = pytest.mark.gpu

POOL_BYTES = 35 * 2 ** 28  # 8.75 GiB: the widest case (far float32 rows of crf_greedy_search) maps 8.63 GiB
REPORT = {}


@pytest.fixture(scope="module")
def state():
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip("%.1f GiB of device memory free: the far-offset table wants 24 GiB" % (free / 2.0 ** 30))
    torch.cuda.reset_peak_memory_stats()
    st = {"env": F.Env("cuda", None)}
    yield st
    st["env"].close()
    print("far offsets: peak torch.cuda.max_memory_allocated() = %.2f GiB; handle workspace at its largest = %d bytes; "
          "slowest case %.2f s (%s)" % (torch.cuda.max_memory_allocated() / 2.0 ** 30, REPORT.get("workspace", 0),
                                        REPORT.get("slowest", (0.0, ""))[0], REPORT.get("slowest", (0.0, ""))[1]))


def with_pool(state, nbytes):
    """the module's Env on a pool of nbytes: the pool at hand if it has that size, else that one is freed first"""
    import torch
    e = state["env"]
    if e.pool is None or e.pool.numel() != nbytes:
        e.reset()
        e.pool = None
        torch.cuda.empty_cache()
        e.pool = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    return e


@pytest.fixture
def env(state, request):
    e = with_pool(state, POOL_BYTES)
    t0 = time.time()
    yield e
    e.reset()
    dt = time.time() - t0
    if dt > REPORT.get("slowest", (0.0, ""))[0]:
        REPORT["slowest"] = (dt, request.node.name)
    REPORT["workspace"] = max(REPORT.get("workspace", 0), e.workspace_bytes())


NAMES = [s for s in F.SEARCHES if not s.startswith(("nbest2", "crf_nbest2"))]
FAR_READS = [(s, dt, sr, T) for s in NAMES for dt, sr, emu_only in F.FAR_READS if not emu_only for T in F.TS
             if F.crf_T(F.SEARCHES[s], T) == T]


@pytest.mark.parametrize("name,dtype,stride_read,T", FAR_READS, ids=["%s-%s-%d-t%d" % c for c in FAR_READS])
def test_far_reads(env, name, dtype, stride_read, T):
    F.far_reads_case(env, F.SEARCHES[name], dtype, stride_read, T)


@pytest.mark.parametrize("name", NAMES)
def test_far_rows(env, name):
    F.far_rows_case(env, F.SEARCHES[name])


FAR_OUT = [(s, T) for s in F.SEARCHES if not s.startswith(("nbest_", "crf_nbest_")) for T in F.TS if F.crf_T(F.SEARCHES[s], T) == T]


@pytest.mark.parametrize("name,T", FAR_OUT, ids=["%s-t%d" % c for c in FAR_OUT])
def test_far_outputs(env, name, T):
    """labels alone at out_stride 2^32 + 4, then path and quality at 2^30 + 4: no array passes about 4 GiB.  The n-best rows
    r * n_best + i: one read, two hypotheses, so that row 1 is the far one at these strides"""
    s = F.SEARCHES[name]
    F.far_outputs_case(env, s, [(2 ** 32 + 4, False, False), (2 ** 30 + 4, True, True)], T=T, B=1 if s.nbest else 2)


# y.stride per family, within the pool: labels row 1 above 2^32 bytes and 2^31 elements (score, exact mode: no path);
# path / start / count / qual row 1 above 2^32 bytes (2^30 + 4) and above 2^31 elements (2^31 + 4: a span of 8 GiB); post and insertion row 1 above 2^32 bytes (2^28 + 4) and
# above 2^31 elements (2^29 + 4: a span of 8 GiB).  deletion's far row needs 2^30 + 4 and with it 16 GiB of insertion:
# the emulator twin has it
def y_strides(family, band):
    return {"score": (2 ** 30 + 4,) if band else (2 ** 32 + 4,), "align": (2 ** 30 + 4, 2 ** 31 + 4), "posterior": (2 ** 28 + 4, 2 ** 29 + 4),
            "edits": (2 ** 28 + 4, 2 ** 29 + 4)}[family]


LATTICE = [(kind, fam, band, B, n_hyp, ys) for kind in ("ctc", "crf") for fam in F.FAMILIES for band in (0, 6)
           for B, n_hyp in ((2, 1), (1, 2)) for ys in y_strides(fam, band)]


@pytest.mark.parametrize("kind,family,band,B,n_hyp,y_stride", LATTICE, ids=["%s_%s-band%d-b%dh%d-%d" % c for c in LATTICE])
def test_far_labellings(env, kind, family, band, B, n_hyp, y_stride):
    F.lattice_far_case(env, kind, family, band, B, n_hyp, y_stride)


LATTICE_300 = [(kind, fam, band, y_strides(fam, band)[0]) for kind, fam, band in F.LATTICE_300]


@pytest.mark.parametrize("kind,family,band,y_stride", LATTICE_300, ids=["%s_%s-band%d-%d" % c for c in LATTICE_300])
def test_far_labellings_t300(env, kind, family, band, y_stride):
    """T = 300: labellings of about 150 labels, windows that cross 256 rows at the far address"""
    F.lattice_far_case(env, kind, family, band, 2, 1, y_stride, T=300)


@pytest.mark.parametrize("T", F.TS)
@pytest.mark.parametrize("out_stride", [2 ** 30 + 4, 65536 + 4])
def test_far_pack(env, out_stride, T):
    F.pack_case(env, out_stride, T)


@pytest.mark.parametrize("dtype,stride_read", [(dt, sr) for dt, sr, emu_only in F.FAR_READS if not emu_only])
@pytest.mark.parametrize("T", F.TS)
def test_far_session(env, dtype, stride_read, T):
    F.session_case(env, dtype, stride_read, T)


@pytest.mark.parametrize("crf", [False, True], ids=["plain", "crf"])
@pytest.mark.parametrize("which", [1, 2], ids=["any_shape", "slots"])
@pytest.mark.parametrize("mode", [0, 1], ids=["logsumexp", "max"])
@pytest.mark.parametrize("dtype,stride_read,T1", F.DUPLEX_LAYOUTS, ids=["%s-%s-t%d" % c for c in F.DUPLEX_LAYOUTS])
def test_far_duplex(env, crf, which, mode, dtype, stride_read, T1):
    """both batches far: two spans of 4 GiB (stride_read None: far ROWS, time-major, two spans of 4.3 GiB)"""
    F.duplex_case(env, crf, which, mode, dtype, stride_read, T1)


def test_far_envelope(env):
    F.envelope_case(env, 2 ** 30 + 4, 2 ** 28 + 4)


# ---- an arena above 4 GiB ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,beam", [("lane", 64), ("wave", 5), ("generic", 24)])
def test_arena_above_4_gib(state, kernel, beam):
    env = with_pool(state, 2 ** 30)
    t0 = time.time()
    T, want, ws = F.arena_case(env, kernel, beam, overlap=8 if kernel == "generic" else 0)
    env.reset()
    dt = time.time() - t0
    print("arena: %s kernel, beam %d, B = %d, T = %d: %.2f GiB by the formula, workspace %.2f GiB, %.2f s"
          % (kernel, beam, F.ARENA_B, T, want / 2.0 ** 30, ws / 2.0 ** 30, dt))
    if dt > REPORT.get("slowest", (0.0, ""))[0]:
        REPORT["slowest"] = (dt, "test_arena_above_4_gib[%s]" % kernel)
    REPORT["workspace"] = max(REPORT.get("workspace", 0), ws)
    assert dt < 20.0, "an arena case is meant to take a few seconds (1.4 to 2.9 s on an idle MI355X)"
