"""CPU-side twin of tests/test_gpu_far_offsets.py: every entry point of the C ABI, compiled against tests/hipemu's lockstep
wave64 emulation, on layouts whose element offsets pass 2^31 and whose byte offsets pass 2^32 (tests/far_offset_cases.py:
the table, the builders and the checkers).  The backing arrays are np.empty and only the rows a case reads are ever
written, so the gaps are never committed; the largest single array is 16 GiB of virtual memory.

Beside the searches, sessions, duplex searches, the band estimator and pack / unpack: the ten lattice entry points with far
labellings, far reads and far rows, the occupancy blocks far apart and interleaved with far rows, and the two walks over all
labellings with each stride far alone.  The emulator also maps what the GPU's pool cannot: offsets past 2^32 ELEMENTS of
float32 (three occupancy blocks, time-major occupancy rows 2^26 + 8 apart), where an offset kept in 32 unsigned bits wraps.
test_every_dev_entry_point_is_in_the_table holds include/fcd.h to the table: every fcd_*_dev is covered or exempt with a
reason.

The launch log says which instantiation a far call launched: a dispatch change cannot quietly turn the table into a test
of the strided fallbacks; for the lattice families and the walks the far call must launch exactly what the compact call did."""
import ctypes as C

import numpy as np
import pytest

import far_offset_cases as F
import instantiation_cases as IC
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def env():
    with emulated_kernels() as lib:
        lib.hipemu_launch_log_read.restype = C.c_size_t
        lib.hipemu_launch_log_read.argtypes = [C.c_char_p, C.c_size_t]
        e = F.Env()
        e.emu = lib
        yield e
        e.close()


def launched(env):
    """the canonical names launched since the last look"""
    need = env.emu.hipemu_launch_log_read(None, 0)
    buf = C.create_string_buffer(need)
    assert env.emu.hipemu_launch_log_read(buf, need) == need
    env.emu.hipemu_launch_log_reset()
    return {IC.canonical(l) for l in buf.value.decode().splitlines() if l}


def templates(names):
    return {IC.parse(n)[0] for n in names}


# the instantiations a FAR call must launch: aligned far reads take the streaming kernels, + 17 the strided fallbacks
WAVE, LANE, GENERIC = "beam_wave_kernel", "beam_lane_kernel", "beam_generic_kernel"
BEAM_KERNEL = {5: WAVE, 24: LANE, 100: GENERIC}


def expect_far_reads(s, dtype, aligned, got):
    t = templates(got)
    if isinstance(s, F.Viterbi):
        want = "viterbi_stream_kernel<5,%d>" % F.DTYPE_CODE[dtype] if aligned else "viterbi_kernel"
        assert want in got and not ({"viterbi_stream_kernel", "viterbi_tm_kernel", "viterbi_kernel"} & t) - {IC.parse(want)[0]}, got
    elif isinstance(s, F.Beam):
        assert BEAM_KERNEL[s.beam] in t and not ({WAVE, LANE, GENERIC} & t) - {BEAM_KERNEL[s.beam]}, got
    elif isinstance(s, F.CrfBeam):
        assert WAVE in t, got
    elif isinstance(s, F.CrfGreedy):
        # (the streaming kernel takes float32 rows of up to 32 elements; everything else walks serially)
        assert t == {"crf_greedy_stream_kernel" if aligned and s.S <= 8 and dtype == "f32" else "crf_greedy_kernel"}, got
    elif isinstance(s, F.CrfViterbi):
        assert t == {"crf_viterbi_kernel"}, got


# (crf_viterbi_search at S = 256 stays at T = 70, far_offset_cases.crf_T: no second id for the same case)
FAR_READS = [(s, dt, sr, T) for s in F.SEARCHES if not s.startswith(("nbest2", "crf_nbest2"))
             for dt, sr, _ in F.FAR_READS for T in F.TS if F.crf_T(F.SEARCHES[s], T) == T]


@pytest.mark.parametrize("name,dtype,stride_read,T", FAR_READS, ids=["%s-%s-%d-t%d" % c for c in FAR_READS])
def test_far_reads(env, name, dtype, stride_read, T):
    s = F.SEARCHES[name]
    d = s.data(2, F.crf_T(s, T), dtype)
    compact = s.run(env, d)
    s.check(compact, d)
    launched(env)
    far = s.run(env, d, F.Layout(stride_read=stride_read))
    expect_far_reads(s, dtype, stride_read % 8 == 0, launched(env))
    F.assert_same(far, compact, (name, dtype, stride_read, T))


# ---- far rows: time-major, stride_t = 2^25 + 8 elements, T = 70: rows 64 .. 69 lie above 2^31 elements ------------------
FAR_ROWS = [s for s in F.SEARCHES if not s.startswith(("nbest2", "crf_nbest2"))]


@pytest.mark.parametrize("name", FAR_ROWS)
def test_far_rows(env, name):
    """B = 9: viterbi_tm_kernel takes eight reads and the strided kernel the ninth, crf_greedy_stream_kernel<S, true> two
    groups of four and the serial walk the tail"""
    s = F.SEARCHES[name]
    dtype = F.far_rows_dtype(s)
    d = s.data(9, 70, dtype)
    compact = s.run(env, d)
    s.check(compact, d)
    launched(env)
    far = s.run(env, d, F.Layout(stride_read=s.S * F.N, stride_t=F.FAR_ROW_STRIDE))
    got = launched(env)
    if isinstance(s, F.Viterbi):
        assert {"viterbi_tm_kernel<5,1>", "viterbi_kernel"} <= got and "viterbi_stream_kernel" not in templates(got), got
    elif isinstance(s, F.CrfGreedy) and s.S <= 8:
        assert {"crf_greedy_stream_kernel<%d,true>" % s.S, "crf_greedy_kernel"} <= got, got
    F.assert_same(far, compact, (name, "far rows"))


# ---- far outputs: out_stride = 2^32 + 4 for labels, path and quality together ------------------------------------------
FAR_OUT = [(s, T) for s in F.SEARCHES if not s.startswith(("nbest_", "crf_nbest_")) for T in F.TS if F.crf_T(F.SEARCHES[s], T) == T]


@pytest.mark.parametrize("name,T", FAR_OUT, ids=["%s-t%d" % c for c in FAR_OUT])
def test_far_outputs(env, name, T):
    """the n-best rows r * n_best + i: one read, two hypotheses -- row 1 is the far one, and the shared span stays at 16 GiB"""
    s = F.SEARCHES[name]
    F.far_outputs_case(env, s, [(2 ** 32 + 4, True, True)], T=T, B=1 if s.nbest else 2)


# ---- far labellings and lattice outputs --------------------------------------------------------------------------------
# y.stride per family: the emulator maps what the GPU cannot (tests/test_gpu_far_offsets.py) -- post and insertion row 1
# above 2^31 elements (2^29 + 4), deletion row 1 above 2^32 bytes (2^30 + 4), labels row 1 above both (2^32 + 4)
Y_STRIDES = {"score": (2 ** 32 + 4,), "align": (2 ** 30 + 4, 2 ** 31 + 4), "posterior": (2 ** 29 + 4,), "edits": (2 ** 29 + 4, 2 ** 30 + 4)}
LATTICE = [(kind, fam, band, B, n_hyp, ys) for kind in ("ctc", "crf") for fam in F.FAMILIES for band in (0, 6)
           for B, n_hyp in ((2, 1), (1, 2)) for ys in Y_STRIDES[fam]]


@pytest.mark.parametrize("kind,family,band,B,n_hyp,y_stride", LATTICE, ids=["%s_%s-band%d-b%dh%d-%d" % c for c in LATTICE])
def test_far_labellings(env, kind, family, band, B, n_hyp, y_stride):
    F.lattice_far_case(env, kind, family, band, B, n_hyp, y_stride)


LATTICE_300 = [(kind, fam, band, Y_STRIDES[fam][0]) for kind, fam, band in F.LATTICE_300]


@pytest.mark.parametrize("kind,family,band,y_stride", LATTICE_300, ids=["%s_%s-band%d-%d" % c for c in LATTICE_300])
def test_far_labellings_t300(env, kind, family, band, y_stride):
    """T = 300: labellings of about 150 labels, windows that cross 256 rows at the far address"""
    F.lattice_far_case(env, kind, family, band, 2, 1, y_stride, T=300)


# ---- far reads and far rows under the lattice families: labellings and outputs compact ----------------------------------
LATTICE_READS = [(kind, fam, band, dt, sr, B) for kind in ("ctc", "crf") for fam in F.ALL_FAMILIES for band in (0, 6)
                 for dt, sr, B in F.LATTICE_FAR_READS]


@pytest.mark.parametrize("kind,family,band,dtype,stride_read,B", LATTICE_READS, ids=["%s_%s-band%d-%s-%d-b%d" % c for c in LATTICE_READS])
def test_far_lattice_reads(env, kind, family, band, dtype, stride_read, B):
    """read 1 starts stride_read elements behind read 0 (+ 17: elements that are not 8-aligned take other load paths); B = 3:
    read 2 starts above 2^32 elements"""
    F.lattice_far_case(env, kind, family, band, B, 1, layout=F.Layout(stride_read=stride_read), dtype=dtype, launched=lambda: launched(env))


LATTICE_ROWS = [(kind, fam, band, st) for kind in ("ctc", "crf") for fam in F.ALL_FAMILIES for band in (0, 6)
                for st in (F.FAR_ROW_STRIDE, F.FAR_ROW_STRIDE_32)]


@pytest.mark.parametrize("kind,family,band,stride_t", LATTICE_ROWS, ids=["%s_%s-band%d-%d" % c for c in LATTICE_ROWS])
def test_far_lattice_rows(env, kind, family, band, stride_t):
    """time-major, float16, T = 70, read 1 ragged: stride_t = 2^25 + 8 puts rows 64 .. 69 above 2^31 elements, 2^26 + 8 above
    2^32"""
    S = 4 if kind == "crf" else 1
    F.lattice_far_case(env, kind, family, band, 2, 1, layout=F.Layout(stride_read=S * F.N, stride_t=stride_t), dtype="f16",
                       launched=lambda: launched(env))


# ---- the occupancy blocks: whole blocks far apart, and interleaved with far rows ----------------------------------------
OCC_BLOCKS = [(kind, band, B, n_hyp, acc) for kind in ("ctc", "crf") for band in (0, 6) for B, n_hyp in ((2, 1), (1, 2)) for acc in (0, 1)]


@pytest.mark.parametrize("kind,band,B,n_hyp,accumulate", OCC_BLOCKS, ids=["%s-band%d-b%dh%d-acc%d" % c for c in OCC_BLOCKS])
def test_far_occupancy_blocks(env, kind, band, B, n_hyp, accumulate):
    """dense rows (stride_t = S N: crfp_occ_walk's dense clear), block 1 stride_row = 2^31 + 4 floats behind block 0"""
    F.lattice_far_case(env, kind, "occupancy", band, B, n_hyp, occ=F.OccLayout(stride_row=F.OCC_FAR_ROW, accumulate=accumulate),
                       launched=lambda: launched(env))


OCC_ROWS = [(kind, band, pad, acc) for kind in ("ctc", "crf") for band in (0, 6) for pad, acc in ((0, 0), (0, 1), (4, 0))]


@pytest.mark.parametrize("kind,band,pad,accumulate", OCC_ROWS, ids=["%s-band%d-pad%d-acc%d" % c for c in OCC_ROWS])
def test_far_occupancy_rows(env, kind, band, pad, accumulate):
    """the time-major layout of a training step: stride_row = S N (+ pad), stride_t = 2^25 + 8 floats, two reads, T = 70 --
    rows 64 .. 69 of both blocks above 2^31 elements (the strided clear and the row stores)"""
    SN = (4 if kind == "crf" else 1) * F.N
    F.lattice_far_case(env, kind, "occupancy", band, 2, 1, occ=F.OccLayout(stride_row=SN + pad, stride_t=F.OCC_FAR_T, accumulate=accumulate),
                       launched=lambda: launched(env))


@pytest.mark.parametrize("kind", ["ctc", "crf"])
def test_far_occupancy_t300(env, kind):
    """T = 300 under the band, as the posterior and edits families (far_offset_cases.LATTICE_300)"""
    F.lattice_far_case(env, kind, "occupancy", 6, 2, 1, T=300, occ=F.OccLayout(stride_row=F.OCC_FAR_ROW), launched=lambda: launched(env))


@pytest.mark.parametrize("kind", ["ctc", "crf"])
@pytest.mark.parametrize("band", [0, 6])
def test_far_occupancy_beyond_2_32_elements(env, kind, band):
    """what only the emulator can map (16 GiB each): three dense blocks, block 2 above 2^32 floats; and time-major rows
    2^26 + 8 floats apart at T = 65, row 64 above 2^32 floats -- where an offset kept in 32 unsigned bits wraps"""
    F.lattice_far_case(env, kind, "occupancy", band, 3, 1, occ=F.OccLayout(stride_row=F.OCC_FAR_ROW), launched=lambda: launched(env))
    SN = (4 if kind == "crf" else 1) * F.N
    F.lattice_far_case(env, kind, "occupancy", band, 2, 1, T=65, occ=F.OccLayout(stride_row=SN, stride_t=F.FAR_ROW_STRIDE_32),
                       launched=lambda: launched(env))


@pytest.mark.parametrize("kind", ["ctc", "crf"])
@pytest.mark.parametrize("band", [0, 6])
def test_far_occupancy_one_read_per_group(env, kind, band):
    F.occupancy_grouped_case(env, kind, band)


@pytest.mark.parametrize("kind", ["ctc", "crf"])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_far_occupancy_no_value(env, kind, accumulate):
    F.occupancy_no_value_case(env, kind, accumulate)


# ---- the walks over all labellings ---------------------------------------------------------------------------------------
WALKS = F.walk_table(gpu=False)


@pytest.mark.parametrize("which,S,T,axis,stride,dtype,layout,out", WALKS, ids=[F.walk_id(c) for c in WALKS])
def test_far_walks(env, which, S, T, axis, stride, dtype, layout, out):
    F.walk_far_case(env, which, S, T, axis, stride, dtype, layout, out, launched=lambda: launched(env))


# ---- every entry point ---------------------------------------------------------------------------------------------------
def test_every_dev_entry_point_is_in_the_table():
    """include/fcd.h against far_offset_cases.COVERED / EXEMPT: an entry point added without a far case fails here"""
    import os
    import re
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "fcd.h")
    with open(header) as f:
        names = set(re.findall(r"\b(fcd_\w+_dev\w*)\s*\(", f.read()))
    assert len(names) >= 30, sorted(names)
    assert not set(F.COVERED) & set(F.EXEMPT)
    missing = sorted(names - set(F.COVERED) - set(F.EXEMPT))
    assert not missing, ("no far-offset case and no exemption", missing)
    stale = sorted((set(F.COVERED) | set(F.EXEMPT)) - names)
    assert not stale, ("not declared in include/fcd.h", stale)
    for name, axes in F.COVERED.items():
        assert axes and all(isinstance(a, str) and a for a in axes), name
    for name, reason in F.EXEMPT.items():
        assert isinstance(reason, str) and len(reason) > 20 and "\n" not in reason, name


# ---- pack / offsets / unpack -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", F.TS)
@pytest.mark.parametrize("out_stride", [2 ** 30 + 4, 65536 + 4])
def test_far_pack(env, out_stride, T):
    F.pack_case(env, out_stride, T)


# ---- sessions, the duplex searches and the band estimator from far buffers ---------------------------------------------
@pytest.mark.parametrize("T", F.TS)
@pytest.mark.parametrize("dtype,stride_read", [(dt, sr) for dt, sr, _ in F.FAR_READS])
def test_far_session(env, dtype, stride_read, T):
    F.session_case(env, dtype, stride_read, T)


@pytest.mark.parametrize("crf", [False, True], ids=["plain", "crf"])
@pytest.mark.parametrize("which", [1, 2], ids=["any_shape", "slots"])
@pytest.mark.parametrize("mode", [0, 1], ids=["logsumexp", "max"])
@pytest.mark.parametrize("dtype,stride_read,T1", F.DUPLEX_LAYOUTS, ids=["%s-%s-t%d" % c for c in F.DUPLEX_LAYOUTS])
def test_far_duplex(env, crf, which, mode, dtype, stride_read, T1):
    """stride_read None: far ROWS, time-major with stride_t = 2^25 + 8"""
    launched(env)
    F.duplex_case(env, crf, which, mode, dtype, stride_read, T1)
    t = templates(launched(env))
    assert ("duplex_slots_kernel" if which == 2 else "duplex_kernel") in t and not ("duplex_kernel" if which == 2 else "duplex_slots_kernel") in t, t


def test_far_envelope(env):
    F.envelope_case(env, 2 ** 30 + 4, 2 ** 28 + 4)
