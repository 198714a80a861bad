"""CPU-side check of the CRF edge-occupancy walk (csrc/crf_posterior.hip, crfp_occ_walk inside crfp_back_kernel<K, 2, 4>,
compiled against tests/hipemu's lockstep wave64 emulation) through crf_occupancy_batch_raw on numpy, against the float64
restatement tests/crf_occupancy_reference.py: the table of tests/crf_occupancy_cases.py (T = 1, a homopolymer's colliding
entries, 1 / 2 / 4 / 8 states per lane, a band across a tile, S = 16 / 64 / 256 / 1024 / 3 / 5, f16 / bf16, time-major and
padded strides, both accumulate modes, P = 0, a NaN, L > T_r) with the launch log showing the instantiations each case ran;
the argument errors and limits at both layers; the results' own crf_occupancy; the single-read function; and a workspace
limit that forces several groups.  The -m gpu twin is tests/test_gpu_crf_occupancy.py."""
import ctypes as C
import math

import numpy as np
import pytest

import crf_lattice_cases as CC
import crf_occupancy_cases as OC
import crf_occupancy_reference as O
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


@pytest.mark.parametrize("case", OC.CASES, ids=[c["name"] for c in OC.CASES])
def test_against_restatement(emu, case):
    fcd, lib = emu
    c = OC.build_case(case)
    lib.hipemu_launch_log_reset()
    OC.run_case(fcd, c)
    ran = {n for n in launched(lib) if n.startswith("crfp_")}
    assert ran == {"crfp_fwd_kernel<%d>" % c["k"], "crfp_back_kernel<%d,2,4>" % c["k"]}, ran


def test_allocated_outputs(fcd):
    """out=None: zeros where nothing is written, (B, n_hyp, T, S, N); time_major_out: the view of a (T, B, n_hyp, S, N) array"""
    c = OC.build_case(OC.CASES[7])
    args = (c["xin"], c["init"], c["labels"], c["out_len"], c["lengths"])
    a = fcd.crf_occupancy_batch_raw(*args, n_valid=c["n_valid"])
    t = fcd.crf_occupancy_batch_raw(*args, n_valid=c["n_valid"], time_major_out=True)
    assert a.occupancy.shape == (3, 2, c["T"], c["S"], c["N"]) and a.occupancy.flags.c_contiguous
    assert t.occupancy.shape == a.occupancy.shape and t.occupancy.transpose(2, 0, 1, 3, 4).flags.c_contiguous
    assert np.array_equal(a.occupancy, t.occupancy) and np.array_equal(a.logp, t.logp, equal_nan=True)
    assert (a.occupancy[1, 0, c["T"] - 3:] == 0).all() and (a.occupancy[1, 1] == 0).all() and (a.occupancy[2] == 0).all()
    assert a.cpu() is a
    OC.check(c, a.occupancy, a.logp, fcd.crf_score_batch_raw(*args, n_valid=c["n_valid"]), np.zeros_like(a.occupancy))
    # one labelling per read: a (B, T, S, N) buffer, the shape of crf_marginals_batch_raw's marginals
    buf = np.zeros((3, c["T"], c["S"], c["N"]), np.float32)
    one = fcd.crf_occupancy_batch_raw(c["xin"], c["init"], c["labels"][:, 0], c["out_len"][:, 0], c["lengths"], out=buf)
    assert one.occupancy is buf and np.array_equal(buf, a.occupancy[:, 0])


def test_argument_errors_and_limits(fcd):
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(6)
    x = CC.posteriors(rng, 2, 10, 4, 5)
    init = np.ones((2, 4), np.float32)
    labels = np.ones((2, 10), np.uint8)
    lens = np.array([3, 4], np.uint32)
    f = fcd.crf_occupancy_batch_raw
    with pytest.raises(ValueError):
        f(x, init, labels, lens, band=-1)
    with pytest.raises(ValueError):
        f(x, init, labels, lens, band=4)  # no paths
    with pytest.raises(ValueError):
        f(x, init, labels, lens, accumulate=True)  # nothing to add to
    with pytest.raises(ValueError):
        f(x, init, labels, lens, out=np.zeros((2, 10, 4, 5), np.float32), time_major_out=True)
    with pytest.raises(ValueError):
        f(x, init, labels, lens, out=np.zeros((2, 9, 4, 5), np.float32))
    with pytest.raises(TypeError):
        f(x, init, labels, lens, out=np.zeros((2, 10, 4, 5), np.float64))
    with pytest.raises(ValueError):
        f(x, init, labels, lens, out=np.zeros((2, 10, 4, 6), np.float32)[..., :5])  # rows that are not dense
    with pytest.raises(ValueError):
        f(x, init, labels[:1], lens)
    # the C ABI refuses them itself, before anything is enqueued or written
    h = nat.default_handle()
    path = np.zeros((2, 10), np.uint32)
    oc, lp = np.full((2, 10, 4, 5), 77.0, np.float32), np.full(2, 77.0)

    def call(fn, S=4, n_hyp=1, band=0, with_path=True, occ=True, logp=True, with_init=True, out=True, stride_t=20, stride_row=200,
             accumulate=0):
        b = nat.Batch(x.ctypes.data, 2, 10, S, 5, 200, 20, 5, 1, None)
        y = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, path.ctypes.data if with_path else None, n_hyp, 10)
        o = nat.Occupancy(oc.ctypes.data if occ else None, stride_row, stride_t, 1.0, accumulate, lp.ctypes.data if logp else None)
        return getattr(h.lib, fn)(h.ptr, C.byref(b), init.ctypes.data if with_init else None, 4, 4, C.byref(y), band,
                                  C.byref(o) if out else None)
    for fn in ("fcd_crf_occupancy_host", "fcd_crf_occupancy_dev"):
        assert call(fn, band=-1) == nat.E_INVALID
        assert call(fn, band=3, with_path=False) == nat.E_INVALID
        assert call(fn, n_hyp=0) == nat.E_INVALID
        assert call(fn, S=0) == nat.E_INVALID
        assert call(fn, with_init=False) == nat.E_INVALID
        assert call(fn, out=False) == nat.E_INVALID
        assert call(fn, occ=False) == nat.E_INVALID
        assert call(fn, stride_t=19) == nat.E_INVALID
        assert call(fn, stride_row=-1) == nat.E_INVALID
        assert call(fn, accumulate=2) == nat.E_INVALID
        assert call(fn, stride_row=0) == nat.E_INVALID and b"overlap" in h.lib.fcd_last_error(h.ptr)
        assert call(fn, stride_row=199) == nat.E_INVALID  # the second block starts inside the first
        assert call(fn, stride_row=20, stride_t=39) == nat.E_INVALID  # interleaved, and a row too close
    assert (oc == 77).all() and (lp == 77).all()
    assert call("fcd_crf_occupancy_host", logp=False) == nat.OK and (lp == 77).all()
    assert np.abs(oc[0, :, :, :].sum((1, 2)) - 1).max() < 1e-5
    assert call("fcd_crf_occupancy_host") == nat.OK and np.isfinite(lp).all()
    # the limits: a window of 513 states, and an S * N row beyond the LDS of a workgroup; the largest shapes inside them
    for T, S, N, band, msg in ((512, 4, 5, 0, b"exceeds 512 states: use a band"), (600, 4, 5, 256, b"exceeds 512 states: use a narrower band"),
                               (8, 8192, 5, 0, b"crf_occupancy: the labelling and the S * N accumulation row do not fit the 160 KiB"),
                               (8, 16, 10, 0, b"crf_occupancy: more than 8 labels")):
        for fn in ("fcd_crf_occupancy_host", "fcd_crf_occupancy_dev"):
            b = nat.Batch(None, 0, T, S, N, T * S * N, S * N, N, 1, None)
            y = nat.Labellings(None, None, None, path.ctypes.data, 1, T)
            o = nat.Occupancy(None, T * S * N, S * N, 1.0, 0, None)
            assert getattr(h.lib, fn)(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(y), band, C.byref(o)) == nat.E_UNSUPPORTED
            assert msg in h.lib.fcd_last_error(h.ptr), h.lib.fcd_last_error(h.ptr)
    for T, S, N, band in ((511, 4, 5, 0), (600, 16, 5, 255), (8, 1024, 5, 0), (8, 4096, 5, 0), (8, 7960, 5, 0), (8, 5, 4, 0)):
        b = nat.Batch(None, 0, T, S, N, T * S * N, S * N, N, 1, None)
        y = nat.Labellings(None, None, None, path.ctypes.data, 1, T)
        o = nat.Occupancy(None, T * S * N, S * N, 1.0, 0, None)
        assert h.lib.fcd_crf_occupancy_host(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(y), band, C.byref(o)) == nat.OK, (T, S, N)
    with pytest.raises(nat.NativeError) as e:
        f(np.zeros((1, 1, 8192, 5), np.float32), np.ones((1, 8192), np.float32), np.ones((1, 1), np.uint8), [0])
    assert e.value.code == nat.E_UNSUPPORTED and "crf_occupancy" in str(e.value) and "160 KiB" in str(e.value)
    with pytest.raises(nat.NativeError) as e:
        f(np.zeros((1, 512, 4, 5), np.float32), np.ones((1, 4), np.float32), np.ones((1, 512), np.uint8), [5])
    assert e.value.code == nat.E_UNSUPPORTED and "use a band" in str(e.value)


def test_results_give_their_occupancies(fcd):
    rng = np.random.default_rng(7)
    x = CC.posteriors(rng, 4, 40, 4, 5)
    init = rng.random((4, 4)).astype(np.float32)
    lengths = np.array([40, 23, 1, 36], np.int64)
    r = fcd.crf_beam_search_batch_raw(x, init, 5, 0.0, lengths=lengths)
    for band in (0, 4):
        got = r.crf_occupancy(x, init, lengths=lengths, band=band)
        assert got.occupancy.shape == (4, 1, 40, 4, 5) and got.logp.shape == (4, 1)
        assert np.array_equal(got.logp, r.crf_score(x, init, lengths=lengths, band=band))
        for b in range(4):
            n, Tr = int(r.out_len[b]), int(lengths[b])
            ref = O.occupancy64(x[b, :Tr], init[b], r.labels[b, :n], band, r.path[b, :n] if band else None)
            W = min(n + 1, 2 * band + 1) if band else n + 1
            assert (np.abs(got.occupancy[b, 0, :Tr] - ref["occ"]) <= OC.tolerance(Tr, W, ref["occ"])).all(), (band, b)
            assert (got.occupancy[b, 0, Tr:] == 0).all()
    # (the n-best results: test_workspace_limit_groups)  plain CTC results are refused
    xp = CC.posteriors(rng, 2, 6, 1, 5)[:, :, 0]
    with pytest.raises(ValueError, match="CRF"):
        fcd.beam_search_batch_raw(xp, 5, 0.0).crf_occupancy(xp, init[:2])
    with pytest.raises(ValueError, match="CRF"):
        fcd.beam_search_nbest_batch_raw(xp, 2, 5, 0.0).crf_occupancy(xp, init[:2])


def test_single_read_function(fcd):
    rng = np.random.default_rng(5)
    x = CC.posteriors(rng, 1, 30, 4, 5)[0]
    init = rng.random(4).astype(np.float32)
    seq, _ = fcd.crf_beam_search(x, init, "NACGT", 5)
    occ, logp = fcd.crf_occupancy(x, init, seq, "NACGT")
    ref = O.occupancy64(x, init, ["NACGT".index(ch) for ch in seq])
    assert occ.shape == (30, 4, 5) and occ.dtype == np.float32 and isinstance(logp, float)
    assert logp == fcd.crf_score(x, init, seq, "NACGT") and abs(logp - ref["logp"]) <= CC.tolerance(30)
    assert (np.abs(occ - ref["occ"]) <= OC.tolerance(30, len(seq) + 1, ref["occ"])).all()
    empty, lp0 = fcd.crf_occupancy(x, init, "", "NACGT")
    s0 = int(np.argmax(init))
    # L = 0: 1 on (sigma_0, 0) in every row, and nothing else
    assert math.isfinite(lp0) and (np.abs(empty[:, s0, 0] - 1.0) <= OC.tolerance(30, 1, 1.0)).all()
    assert np.count_nonzero(empty) == 30
    with pytest.raises(RuntimeError, match="no alignment"):
        fcd.crf_occupancy(x[:2], init, "ACGT", "NACGT")
    with pytest.raises(ValueError, match="alphabet size"):
        fcd.crf_occupancy(x, init, seq, "NACG")
    with pytest.raises(TypeError):
        fcd.crf_occupancy(x, init, [1, 2], "NACGT")


def test_workspace_limit_groups(fcd):
    OC.workspace_limit_groups(fcd)


def test_unsupported_labellings_hold_or_are_given_up(fcd):
    OC.unsupported_labellings(fcd)
