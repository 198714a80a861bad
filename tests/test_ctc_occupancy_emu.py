"""CPU-side check of the CTC label-occupancy walk (csrc/ctc_posterior.hip, ctc_occ_walk inside post_back_kernel<K, 8>,
compiled against tests/hipemu's lockstep wave64 emulation) through ctc_occupancy_batch_raw on numpy, against the float64
restatement tests/ctc_occupancy_reference.py: the table of tests/ctc_occupancy_cases.py (T = 1, one alignment, a
homopolymer with and without collapse, 2 / 4 / 6 / 8 states per lane, a band across a tile at N = 2 / 5 / 9, a window that
jumps past itself, f16 / bf16, time-major and padded strides, both accumulate modes, P = 0, a NaN on and off the
alignments, a bad label, L > T_r) with the launch log showing the two instantiations each case ran; the argument errors
and limits at both layers; the results' own ctc_occupancy; the single-read function; a workspace limit that forces several
groups; one held and one given-up labelling its read does not support.  The -m gpu twin is tests/test_gpu_ctc_occupancy.py."""
import ctypes as C
import math

import numpy as np
import pytest

import ctc_occupancy_cases as OC
import ctc_occupancy_reference as O
import ctc_score_cases as SC
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
    ran = {n for n in launched(lib) if n.startswith("post_") or n.startswith("edit_")}
    assert ran == {"post_fwd_kernel<%d>" % c["k"], "post_back_kernel<%d,8>" % c["k"]}, ran


def test_allocated_outputs(fcd):
    """out=None: zeros where nothing is written, (B, n_hyp, T, N); time_major_out: the view of a (T, B, n_hyp, N) array"""
    c = OC.build_case(next(k for k in OC.CASES if k["name"] == "n5_t130_band4"))
    args = (c["xin"], c["labels"], c["out_len"], True, c["lengths"], c["paths"], 4)
    a = fcd.ctc_occupancy_batch_raw(*args, n_valid=c["n_valid"])
    t = fcd.ctc_occupancy_batch_raw(*args, n_valid=c["n_valid"], time_major_out=True)
    assert a.occupancy.shape == (3, 2, c["T"], c["N"]) and a.occupancy.flags.c_contiguous
    assert t.occupancy.shape == a.occupancy.shape and t.occupancy.transpose(2, 0, 1, 3).flags.c_contiguous
    assert np.array_equal(a.occupancy, t.occupancy) and np.array_equal(a.logp, t.logp, equal_nan=True)
    assert (a.occupancy[1, 0, c["T"] - 3:] == 0).all() and (a.occupancy[1, 1] == 0).all() and (a.occupancy[2] == 0).all()
    assert a.cpu() is a
    OC.check(c, a.occupancy, a.logp, fcd.ctc_score_batch_raw(*args, n_valid=c["n_valid"]), np.zeros_like(a.occupancy))
    # one labelling per read: a (B, T, N) buffer, the shape of the input
    buf = np.zeros((3, c["T"], c["N"]), np.float32)
    one = fcd.ctc_occupancy_batch_raw(c["xin"], c["labels"][:, 0], c["out_len"][:, 0], True, c["lengths"], c["paths"][:, 0], 4, out=buf)
    assert one.occupancy is buf and np.array_equal(buf, a.occupancy[:, 0])


def test_argument_errors_and_limits(fcd):
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(6)
    x = SC.posteriors(rng, 2, 10, 5)
    labels = np.ones((2, 10), np.uint8)
    lens = np.array([3, 4], np.uint32)
    f = fcd.ctc_occupancy_batch_raw
    with pytest.raises(ValueError):
        f(x, labels, lens, band=-1)
    with pytest.raises(ValueError):
        f(x, labels, lens, band=4)  # no paths
    with pytest.raises(ValueError):
        f(x, labels, lens, accumulate=True)  # nothing to add to
    with pytest.raises(ValueError):
        f(x, labels, lens, out=np.zeros((2, 10, 5), np.float32), time_major_out=True)
    with pytest.raises(ValueError):
        f(x, labels, lens, out=np.zeros((2, 9, 5), np.float32))
    with pytest.raises(TypeError):
        f(x, labels, lens, out=np.zeros((2, 10, 5), np.float64))
    with pytest.raises(ValueError):
        f(x, labels, lens, out=np.zeros((2, 10, 10), np.float32)[..., ::2])  # rows that are not dense
    with pytest.raises(ValueError):
        f(x, labels[:1], lens)
    # the C ABI refuses them itself, before anything is enqueued or written
    h = nat.default_handle()
    path = np.zeros((2, 10), np.uint32)
    oc, lp = np.full((2, 10, 5), 77.0, np.float32), np.full(2, 77.0)

    def call(fn, S=1, n_hyp=1, band=0, with_path=True, occ=True, logp=True, out=True, stride_t=5, stride_row=50, accumulate=0):
        b = nat.Batch(x.ctypes.data, 2, 10, S, 5, 50, 5, 0, 1, None)
        y = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, path.ctypes.data if with_path else None, n_hyp, 10)
        o = nat.Occupancy(oc.ctypes.data if occ else None, stride_row, stride_t, 1.0, accumulate, lp.ctypes.data if logp else None)
        return getattr(h.lib, fn)(h.ptr, C.byref(b), C.byref(y), 1, band, C.byref(o) if out else None)
    for fn in ("fcd_ctc_occupancy_host", "fcd_ctc_occupancy_dev"):
        assert call(fn, band=-1) == nat.E_INVALID
        assert call(fn, band=3, with_path=False) == nat.E_INVALID
        assert call(fn, n_hyp=0) == nat.E_INVALID
        assert call(fn, S=4) == nat.E_INVALID
        assert call(fn, out=False) == nat.E_INVALID and b"ctc_occupancy" in h.lib.fcd_last_error(h.ptr)
        assert call(fn, occ=False) == nat.E_INVALID and b"ctc_occupancy" in h.lib.fcd_last_error(h.ptr)
        assert call(fn, stride_t=4) == nat.E_INVALID and b"ctc_occupancy" in h.lib.fcd_last_error(h.ptr)
        assert call(fn, stride_row=-1) == nat.E_INVALID
        assert call(fn, accumulate=2) == nat.E_INVALID
        assert call(fn, stride_row=0) == nat.E_INVALID and b"overlap" in h.lib.fcd_last_error(h.ptr)
        assert call(fn, stride_row=49) == nat.E_INVALID  # the second block starts inside the first
        assert call(fn, stride_row=5, stride_t=9) == nat.E_INVALID  # interleaved, and a row too close
    assert (oc == 77).all() and (lp == 77).all()
    assert call("fcd_ctc_occupancy_host", logp=False) == nat.OK and (lp == 77).all()
    assert np.abs(oc.sum(2) - 1).max() < 1e-5
    assert call("fcd_ctc_occupancy_host") == nat.OK and np.isfinite(lp).all()
    # the limits: a window of 511 states, 9 labels, a labelling beyond the LDS copy; the largest shapes inside them
    for T, N, band, stride, msg in ((255, 5, 0, 255, b"ctc_occupancy: the exact lattice exceeds 510 states: use a band"),
                                    (600, 5, 127, 600, b"ctc_occupancy: the band's window exceeds 510 states: use a narrower band"),
                                    (8, 10, 0, 8, b"ctc_occupancy: more than 8 labels"),
                                    (28481, 5, 16, 28481, b"ctc_occupancy: labellings beyond 28480 labels")):
        for fn in ("fcd_ctc_occupancy_host", "fcd_ctc_occupancy_dev"):
            b = nat.Batch(None, 0, T, 1, N, T * N, N, 0, 1, None)
            y = nat.Labellings(None, None, None, path.ctypes.data, 1, stride)
            o = nat.Occupancy(None, T * N, N, 1.0, 0, None)
            assert getattr(h.lib, fn)(h.ptr, C.byref(b), C.byref(y), 1, band, C.byref(o)) == nat.E_UNSUPPORTED
            assert msg in h.lib.fcd_last_error(h.ptr), h.lib.fcd_last_error(h.ptr)
    for T, N, band, stride in ((254, 5, 0, 254), (4000, 5, 0, 254), (600, 9, 126, 600), (28480, 2, 16, 28480)):
        b = nat.Batch(None, 0, T, 1, N, T * N, N, 0, 1, None)
        y = nat.Labellings(None, None, None, path.ctypes.data, 1, stride)
        o = nat.Occupancy(None, T * N, N, 1.0, 0, None)
        assert h.lib.fcd_ctc_occupancy_host(h.ptr, C.byref(b), C.byref(y), 1, band, C.byref(o)) == nat.OK, (T, N, band)
    with pytest.raises(nat.NativeError) as e:
        f(np.zeros((1, 255, 5), np.float32), np.ones((1, 255), np.uint8), [5])
    assert e.value.code == nat.E_UNSUPPORTED and "ctc_occupancy" in str(e.value) and "use a band" in str(e.value)


def test_results_give_their_occupancies(fcd):
    rng = np.random.default_rng(7)
    x = SC.posteriors(rng, 4, 40, 5)
    lengths = np.array([40, 23, 1, 36], np.int64)
    r = fcd.beam_search_batch_raw(x, 5, 0.0, lengths=lengths)
    for band in (0, 4):
        got = r.ctc_occupancy(x, lengths=lengths, band=band)
        assert got.occupancy.shape == (4, 1, 40, 5) and got.logp.shape == (4, 1)
        assert np.array_equal(got.logp, r.ctc_score(x, lengths=lengths, band=band))
        K = OC.states_per_lane(40, r.labels.shape[-1], band)
        for b in range(4):
            n, Tr = int(r.out_len[b]), int(lengths[b])
            ref = O.occupancy64(x[b, :Tr], r.labels[b, :n], True, band, r.path[b, :n] if band else None)
            assert (np.abs(got.occupancy[b, 0, :Tr] - ref["occ"]) <= OC.tolerance(Tr, K, ref["occ"])).all(), (band, b)
            assert (got.occupancy[b, 0, Tr:] == 0).all()
    # (the n-best results: test_workspace_limit_groups)  CRF results are refused
    x4 = np.repeat(x[:2, :6, None], 4, axis=2)
    init = np.ones((2, 4), np.float32)
    with pytest.raises(ValueError, match="CRF"):
        fcd.crf_beam_search_batch_raw(x4, init, 5, 0.0).ctc_occupancy(x4)
    with pytest.raises(ValueError, match="CRF"):
        fcd.crf_beam_search_nbest_batch_raw(x4, init, 2, beam_size=5).ctc_occupancy(x[:2, :6])


def test_single_read_function(fcd):
    rng = np.random.default_rng(5)
    x = SC.posteriors(rng, 1, 30, 5)[0]
    seq, _ = fcd.beam_search(x, "NACGT", 5)
    for collapse in (True, False):
        occ, logp = fcd.ctc_occupancy(x, seq, "NACGT", collapse)
        ref = O.occupancy64(x, ["NACGT".index(ch) for ch in seq], collapse)
        assert occ.shape == (30, 5) and occ.dtype == np.float32 and isinstance(logp, float)
        assert logp == fcd.ctc_score(x, seq, "NACGT", collapse) and SC.same(logp, ref["logp"], 30)
        assert (np.abs(occ - ref["occ"]) <= OC.tolerance(30, 2, ref["occ"])).all()
    empty, lp0 = fcd.ctc_occupancy(x, "", "NACGT")
    # L = 0: 1 on the blank in every row, and nothing else
    assert math.isfinite(lp0) and (np.abs(empty[:, 0] - 1.0) <= OC.tolerance(30, 2, 1.0)).all()
    assert np.count_nonzero(empty) == 30
    with pytest.raises(RuntimeError, match="no alignment"):
        fcd.ctc_occupancy(x[:2], "ACGT", "NACGT")
    with pytest.raises(ValueError, match="alphabet size"):
        fcd.ctc_occupancy(x, seq, "NACG")
    with pytest.raises(TypeError):
        fcd.ctc_occupancy(x, [1, 2], "NACGT")


def test_same_bits_twice(fcd):
    c = OC.build_case(next(k for k in OC.CASES if k["name"] == "n9_t193_l190_k6"))
    args = (c["xin"], c["labels"], c["out_len"], True, c["lengths"])
    a, b = fcd.ctc_occupancy_batch_raw(*args), fcd.ctc_occupancy_batch_raw(*args)
    assert np.array_equal(a.occupancy.view(np.uint32), b.occupancy.view(np.uint32))


def test_workspace_limit_groups(fcd):
    OC.workspace_limit_groups(fcd)


def test_unsupported_labellings_hold_or_are_given_up(fcd):
    OC.unsupported_labellings(fcd)
