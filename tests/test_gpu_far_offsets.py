"""GPU twin of tests/test_far_offsets_emu.py: every entry point of the C ABI on device buffers whose element offsets pass
2^31 and whose byte offsets pass 2^32 (tests/far_offset_cases.py: the table, the builders and the checkers) -- where the
kernels' 32-bit address tricks (byte-offset slabs, wave-uniform bases with one vector offset) actually run.  The lattice
families (occupancy included) take far labellings, far reads and far rows, the occupancy blocks lie 8 GiB apart or interleave
with far rows, and the walks over all labellings (crf_transition_probs, crf_marginals) take each of their strides far alone:
ONE far quantity per case.

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


# ---- far reads and far rows under the lattice families: labellings and outputs compact (a span of 4 to 4.3 GiB) ----------
LATTICE_READS = [(kind, fam, band, dt, sr, B) for kind in ("ctc", "crf") for fam in F.ALL_FAMILIES for band in (0, 6)
                 for dt, sr, B in F.LATTICE_FAR_READS_GPU]


@pytest.mark.parametrize("kind,family,band,dtype,stride_read,B", LATTICE_READS, ids=["%s_%s-band%d-%s-%d-b%d" % c for c in LATTICE_READS])
def test_far_lattice_reads(env, kind, family, band, dtype, stride_read, B):
    """B = 3: read 2 starts above 2^32 elements, a span of 8 GiB"""
    F.lattice_far_case(env, kind, family, band, B, 1, layout=F.Layout(stride_read=stride_read), dtype=dtype)


LATTICE_ROWS = [(kind, fam, band, st) for kind in ("ctc", "crf") for fam in F.ALL_FAMILIES for band in (0, 6)
                for st in (F.FAR_ROW_STRIDE, F.FAR_ROW_STRIDE_32)]


@pytest.mark.parametrize("kind,family,band,stride_t", LATTICE_ROWS, ids=["%s_%s-band%d-%d" % c for c in LATTICE_ROWS])
def test_far_lattice_rows(env, kind, family, band, stride_t):
    """time-major, float16, T = 70, read 1 ragged: stride_t = 2^25 + 8 puts rows 64 .. 69 above 2^31 elements, 2^26 + 8 above
    2^32 (8.63 GiB)"""
    S = 4 if kind == "crf" else 1
    F.lattice_far_case(env, kind, family, band, 2, 1, layout=F.Layout(stride_read=S * F.N, stride_t=stride_t), dtype="f16")


# ---- the occupancy blocks: 2^31 + 4 floats apart (a span of 8 GiB), or interleaved with rows 2^25 + 8 floats apart (8.63
# GiB: with far float32 rows of crf_greedy_search the widest span of the table) ---------------------------------------------
OCC_BLOCKS = [(kind, band, B, n_hyp, acc) for kind in ("ctc", "crf") for band in (0, 6) for B, n_hyp in ((2, 1), (1, 2)) for acc in (0, 1)]


@pytest.mark.parametrize("kind,band,B,n_hyp,accumulate", OCC_BLOCKS, ids=["%s-band%d-b%dh%d-acc%d" % c for c in OCC_BLOCKS])
def test_far_occupancy_blocks(env, kind, band, B, n_hyp, accumulate):
    F.lattice_far_case(env, kind, "occupancy", band, B, n_hyp, occ=F.OccLayout(stride_row=F.OCC_FAR_ROW, accumulate=accumulate))


OCC_ROWS = [(kind, band, pad, acc) for kind in ("ctc", "crf") for band in (0, 6) for pad, acc in ((0, 0), (0, 1), (4, 0))]


@pytest.mark.parametrize("kind,band,pad,accumulate", OCC_ROWS, ids=["%s-band%d-pad%d-acc%d" % c for c in OCC_ROWS])
def test_far_occupancy_rows(env, kind, band, pad, accumulate):
    """the time-major layout of a training step: stride_row = S N (+ pad), stride_t far, two reads, T = 70"""
    SN = (4 if kind == "crf" else 1) * F.N
    F.lattice_far_case(env, kind, "occupancy", band, 2, 1, occ=F.OccLayout(stride_row=SN + pad, stride_t=F.OCC_FAR_T, accumulate=accumulate))


@pytest.mark.parametrize("kind", ["ctc", "crf"])
def test_far_occupancy_t300(env, kind):
    F.lattice_far_case(env, kind, "occupancy", 6, 2, 1, T=300, occ=F.OccLayout(stride_row=F.OCC_FAR_ROW))


@pytest.mark.parametrize("kind", ["ctc", "crf"])
@pytest.mark.parametrize("band", [0, 6])
def test_far_occupancy_one_read_per_group(env, kind, band):
    F.occupancy_grouped_case(env, kind, band)


@pytest.mark.parametrize("kind", ["ctc", "crf"])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_far_occupancy_no_value(env, kind, accumulate):
    F.occupancy_no_value_case(env, kind, accumulate)


# ---- the walks over all labellings: one stride far per case; float32 rows of S = 256 at bytes past 2^32 (the emulator twin
# takes them past 2^31 elements, 16 GiB) ------------------------------------------------------------------------------------
WALKS = F.walk_table(gpu=True)


@pytest.mark.parametrize("which,S,T,axis,stride,dtype,layout,out", WALKS, ids=[F.walk_id(c) for c in WALKS])
def test_far_walks(env, which, S, T, axis, stride, dtype, layout, out):
    F.walk_far_case(env, which, S, T, axis, stride, dtype, layout, out)


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
