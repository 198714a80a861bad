"""CPU-side check of the LDS-resident CRF walks (csrc/crf_lattice.h: crf_forward_walk_lds inside crfp_fwd_kernel<8>;
csrc/crf_posterior.hip: crfp_occ_walk_lds inside crfp_back_kernel<8, 2, 4>, compiled against tests/hipemu's lockstep wave64
emulation) through crf_score_batch_raw(wide=True) and crf_occupancy_batch_raw(wide=True) on numpy, against the float64
restatement tests/crf_occupancy_reference.py: the table of tests/crf_occupancy_wide_cases.py with the launch log showing
exactly the two hosting instantiations and the score's bits in the occupancy call's logp; wide=True on register-resident
cases (the launches and the logp bits of wide=False); limits and messages at both layers, nothing written on a refused
call, the 513-state call refused as before with the switch off; a workspace limit that forces several groups; the boundary
of what one exponent per row holds beyond the registers.  The -m gpu twin is tests/test_gpu_crf_occupancy_wide.py."""
import ctypes as C

import numpy as np
import pytest

import crf_occupancy_cases as OC
import crf_occupancy_wide_cases as WC
import instantiation_cases as IC
from emu_util import emulated_kernels


@pytest.fixture(scope="module")
def emu():
    import fast_ctc_decode_amd as m
    with emulated_kernels() as lib:
        lib.hipemu_launch_log_read.restype = C.c_size_t
        lib.hipemu_launch_log_read.argtypes = [C.c_char_p, C.c_size_t]
        yield m, lib


@pytest.fixture(scope="module")
def fcd(emu):
    return emu[0]


def launched(lib):
    need = lib.hipemu_launch_log_read(None, 0)
    buf = C.create_string_buffer(need)
    assert lib.hipemu_launch_log_read(buf, need) == need
    return {IC.canonical(l) for l in buf.value.decode().splitlines() if l}


@pytest.mark.parametrize("case", WC.EMU_CASES, ids=[c["name"] for c in WC.EMU_CASES])
def test_against_restatement(emu, case):
    fcd, lib = emu
    c = WC.build_case(case)
    lib.hipemu_launch_log_reset()
    WC.run_case(fcd, c)  # (the wide score -- the forward kernel, sum only -- then the pair; logp must hold the score's bits)
    ran = {n for n in launched(lib) if n.startswith(("crfp_", "crf_lattice_"))}
    assert ran == WC.LAUNCHES, ran


DELEGATED = ("s4n5_t7_homopolymer", "s4n5_t70_k2", "s4n5_t140_k4", "s4n5_t330_k8", "s4n5_t130_band4")


@pytest.mark.parametrize("name", DELEGATED)
def test_register_windows_are_delegated(emu, name):
    """wide=True where the registers hold the window: the launches of wide=False, logp bit for bit, the occupancies within
    tolerance (their colliding entries are added in LDS in no fixed order, so their bits are not compared)"""
    fcd, lib = emu
    c = OC.build_case(next(k for k in OC.CASES if k["name"] == name))
    args, kw, _ = WC.call_args(c)
    got = []
    for wide in (False, True):
        buf, view, before = OC.out_buffer(c)
        lib.hipemu_launch_log_reset()
        score = fcd.crf_score_batch_raw(*args, wide=wide, **kw)
        r = fcd.crf_occupancy_batch_raw(*args, out=view, wide=wide, **kw)
        ran = {n for n in launched(lib) if n.startswith(("crfp_", "crf_lattice_"))}
        assert ran == {"crf_lattice_kernel<false,%d>" % c["k"], "crfp_fwd_kernel<%d>" % c["k"], "crfp_back_kernel<%d,2,4>" % c["k"]}, (wide, ran)
        OC.check(c, view, r.logp, score, before)
        got.append((score.copy(), r.logp.copy()))
    assert np.array_equal(got[0][0].view(np.uint64), got[1][0].view(np.uint64))
    assert np.array_equal(got[0][1].view(np.uint64), got[1][1].view(np.uint64))


def test_limits_and_messages(fcd):
    from fast_ctc_decode_amd import _native as nat
    h = nat.default_handle()
    path = np.zeros(8, np.uint32)
    init = np.ones((1, 4), np.float32)
    lp = np.full(1, 77.0)

    def call(fn, T, S, N, band, stride=None):
        stride = T if stride is None else stride
        b = nat.Batch(None, 0, T, S, N, T * S * N, S * N, N, 1, None)
        y = nat.Labellings(None, None, None, path.ctypes.data, 1, stride)
        if "occupancy" in fn:
            o = nat.Occupancy(None, T * S * N, S * N, 1.0, 0, None)
            return getattr(h.lib, fn)(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(y), band, C.byref(o))
        return getattr(h.lib, fn)(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(y), band, lp.ctypes.data)
    OCC = ("fcd_crf_occupancy_host", "fcd_crf_occupancy_dev")
    SCORE = ("fcd_crf_score_host", "fcd_crf_score_dev")
    # the switch: 0 or 1; off on a new handle -- 513 states are refused as before, with today's message
    assert h.lib.fcd_set_crf_lattice_wide(h.ptr, 2) == nat.E_INVALID and h.lib.fcd_set_crf_lattice_wide(None, 1) == nat.E_INVALID
    assert h.lib.fcd_set_crf_lattice_wide(h.ptr, -1) == nat.E_INVALID
    for fn in OCC + SCORE:
        assert call(fn, 512, 4, 5, 0) == nat.E_UNSUPPORTED
        assert b"crf lattice: the exact lattice exceeds 512 states: use a band" in h.lib.fcd_last_error(h.ptr)
    # (4 (min(T, stride) + 1) + 4480 + 768 J + 4 S N: S = 7000 at N = 5, 514 states: 2056 + 4480 + 6912 + 140000 = 153448
    # fits, S = 7600 does not -- 165448; the score has no S * N row and takes it)
    refused = ((OCC + SCORE, 4096, 4, 5, 0, b"_wide: the exact lattice exceeds the 4096 states"),
               (OCC + SCORE, 9000, 4, 5, 2048, b"_wide: the band's window exceeds the 4096 states"),
               (OCC + SCORE, 513, 16, 10, 0, b"_wide: more than 8 labels"),
               (OCC + SCORE, 513, 2 ** 24 - 1, 2, 0, b"_wide: S must be below 2^24 - 1"),
               (OCC, 513, 7600, 5, 0, b"_wide: the labelling, the tile, the window's three rows and the S * N accumulation row do not fit"))
    h.set_crf_lattice_wide(True)
    try:
        for fns, T, S, N, band, msg in refused:
            for fn in fns:
                assert call(fn, T, S, N, band) == nat.E_UNSUPPORTED, (fn, T, S, N, band)
                who = b"crf_occupancy" if "occupancy" in fn else b"crf_score"
                assert h.lib.fcd_last_error(h.ptr).startswith(who + msg), h.lib.fcd_last_error(h.ptr)
        assert b"= 165448 bytes" in h.lib.fcd_last_error(h.ptr)
        # the largest shapes inside them; S = 1024 and S = 4096 at N = 5 with 2048 states
        for T, S, N, band in ((512, 4, 5, 0), (4095, 4, 9, 0), (9000, 4, 5, 2047), (2047, 1024, 5, 0), (2047, 4096, 5, 0), (513, 7000, 5, 0)):
            for fn in OCC + SCORE:
                assert call(fn, T, S, N, band) == nat.OK, (fn, T, S, N, band, h.lib.fcd_last_error(h.ptr))
        assert call("fcd_crf_score_host", 513, 7600, 5, 0) == nat.OK
        # every other CRF lattice call ignores the switch
        b = nat.Batch(None, 0, 512, 4, 5, 512 * 20, 20, 5, 1, None)
        y = nat.Labellings(None, None, None, path.ctypes.data, 1, 512)
        al = nat.Alignment(None, None, None, None)
        assert h.lib.fcd_crf_align_host(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(y), 0, C.byref(al)) == nat.E_UNSUPPORTED
        assert b"crf lattice: the exact lattice exceeds 512 states: use a band" in h.lib.fcd_last_error(h.ptr)
    finally:
        h.set_crf_lattice_wide(False)
    for fn in OCC + SCORE:
        assert call(fn, 512, 4, 5, 0) == nat.E_UNSUPPORTED
    assert (lp == 77).all()
    # the Python layer: refused without wide, with the handle's switch off again after an error; nothing is written on a
    # refused call
    c = WC.build_case(WC.CASES[0])
    args, kw, _ = WC.call_args(c)
    buf, view, before = OC.out_buffer(c)
    with pytest.raises(nat.NativeError) as e:
        fcd.crf_occupancy_batch_raw(*args, out=view, **kw)
    assert e.value.code == nat.E_UNSUPPORTED and "exceeds 512 states: use a band" in str(e.value)
    with pytest.raises(nat.NativeError) as e:
        fcd.crf_score_batch_raw(*args, **kw)
    assert e.value.code == nat.E_UNSUPPORTED and "exceeds 512 states: use a band" in str(e.value)
    x10 = np.zeros((1, 513, 4, 10), np.float32)
    big = np.full((1, 1, 513, 4, 10), 77.0, np.float32)
    with pytest.raises(nat.NativeError) as e:
        fcd.crf_occupancy_batch_raw(x10, np.ones((1, 4), np.float32), np.ones((1, 513), np.uint8), [5], out=big, wide=True)
    assert e.value.code == nat.E_UNSUPPORTED and "crf_occupancy_wide: more than 8 labels" in str(e.value)
    with pytest.raises(nat.NativeError) as e:
        fcd.crf_score_batch_raw(x10, np.ones((1, 4), np.float32), np.ones((1, 513), np.uint8), [5], wide=True)
    assert "crf_score_wide: more than 8 labels" in str(e.value)
    assert (view == before).all() and (big == 77.0).all()
    for fn in OCC + SCORE:
        assert call(fn, 512, 4, 5, 0) == nat.E_UNSUPPORTED


def test_results_and_single_read(fcd):
    """the single-read functions with wide=True beyond 511 characters, against the batch call's reference"""
    from fast_ctc_decode_amd import _native as nat
    c = WC.build_case(WC.CASES[0])
    n = int(c["out_len"][0, 0])
    seq = "".join("NACGT"[v] for v in c["labels"][0, 0, :n])
    x, init = c["x32"][0], c["init"][0]
    with pytest.raises(nat.NativeError):
        fcd.crf_score(x, init, seq, "NACGT")
    with pytest.raises(nat.NativeError):
        fcd.crf_occupancy(x, init, seq, "NACGT")
    occ, logp = fcd.crf_occupancy(x, init, seq, "NACGT", wide=True)
    assert logp == fcd.crf_score(x, init, seq, "NACGT", wide=True)
    ref = c["refs"][(0, 0)]
    assert (np.abs(occ - ref["occ"]) <= OC.tolerance(c["T"], n + 1, ref["occ"])).all()


def test_workspace_limit_groups(fcd):
    WC.workspace_limit_groups(fcd)


def test_a_training_chunk_of_an_untrained_network_holds(fcd):
    WC.holds(fcd)


def test_six_rows_per_label_are_given_up(fcd):
    WC.given_up(fcd)
