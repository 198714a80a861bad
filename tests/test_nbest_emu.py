"""CPU-side check of the n-best epilogues of the beam kernels (csrc/beam_wave.hip, beam_lane.hip, beam_generic.hip,
compiled against tests/hipemu's lockstep wave64 emulation): every kernel family, plain and CRF, returns the n best
hypotheses of tests/nbest_reference.py -- labels, paths, bit-exact scores, n_hyp -- and its hypothesis 0 is the
single-result call's, on ragged reads (lengths 0 and 1 included), a NaN read and a threshold that runs out of beam,
under both tie orders.  The -m gpu twin is tests/test_gpu_nbest.py."""
import numpy as np
import pytest

import nbest_cases as NC
from emu_util import emulated_kernels
from tie_util import ORDERS, tie_order


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("N,beam,kernel", NC.PLAIN)
def test_plain_every_family(fcd, N, beam, kernel):
    with tie_order(fcd, "pdq178"):
        NC.run_plain(fcd, N, beam, kernel, stable=False)
        NC.run_plain(fcd, N, beam, kernel, stable=False, thr=0.1, n_best=max(1, beam // 2), seed=1)


@pytest.mark.parametrize("N,S,beam,kernel", NC.CRF)
def test_crf_every_family(fcd, N, S, beam, kernel):
    with tie_order(fcd, "pdq178"):
        NC.run_crf(fcd, N, S, beam, kernel, stable=False)


@pytest.mark.parametrize("N,beam,kernel", [(5, 5, NC.KERNEL_WAVE), (5, 32, NC.KERNEL_LANE), (12, 5, NC.KERNEL_GENERIC)])
def test_stable_tie_order(fcd, N, beam, kernel):
    with tie_order(fcd, "stable"):
        NC.run_plain(fcd, N, beam, kernel, stable=True, seed=2)


@pytest.mark.parametrize("N,beam,kernel", [(5, 5, NC.KERNEL_WAVE), (5, 32, NC.KERNEL_LANE), (12, 5, NC.KERNEL_GENERIC)])
def test_ran_out_of_beam(fcd, N, beam, kernel):
    NC.run_out_of_beam(fcd, N, beam, kernel)


def test_single_read_functions(fcd):
    x, _ = NC.plain_batch(5, 5)
    hyps = fcd.beam_search_nbest(x[0], "NACGT", 3, beam_size=5)
    assert len(hyps) == 3 and all(len(h) == 3 for h in hyps)
    assert hyps[0][:2] == fcd.beam_search(x[0], "NACGT", 5)
    assert hyps[0][2] >= hyps[1][2] >= hyps[2][2]
    with pytest.raises(RuntimeError, match="NaNs"):
        fcd.beam_search_nbest(x[5], "NACGT", 3, beam_size=5)
    xc, init, _ = NC.crf_batch(6, 5, 4)
    hyps = fcd.crf_beam_search_nbest(xc[0], init[0], "NACGT", 5, beam_size=5)
    assert hyps[0][:2] == fcd.crf_beam_search(xc[0], init[0], "NACGT", 5)
    # multi-character labels: the CRF strings follow crf_beam_search's character reversal
    alpha = ["N", "AB", "C", "GT", "T"]
    assert fcd.crf_beam_search_nbest(xc[1], init[1], alpha, 2, beam_size=5)[0][:2] == \
        fcd.crf_beam_search(xc[1], init[1], alpha, 5)


def test_argument_errors(fcd):
    x, _ = NC.plain_batch(5, 5)
    with pytest.raises(ValueError):
        fcd.beam_search_nbest(x[0], "NACGT", 0, beam_size=5)
    with pytest.raises(ValueError):
        fcd.beam_search_nbest(x[0], "NACGT", 6, beam_size=5)
    with pytest.raises(TypeError):
        fcd.beam_search_nbest(x[0], "NACGT", 2.0, beam_size=5)
    with pytest.raises(ValueError, match="alphabet size"):  # the existing checks first, with their messages
        fcd.beam_search_nbest(x[0], "NACG", 2, beam_size=5)
    with pytest.raises(ValueError, match="beam_size cannot be 0"):
        fcd.beam_search_nbest(x[0], "NACGT", 1, beam_size=0)
    with pytest.raises(ValueError):
        fcd.beam_search_nbest_batch_raw(x, 6, 5)
    with pytest.raises(TypeError):
        fcd.beam_search_nbest_batch_raw(x, 1.5, 5)
    xc, init, _ = NC.crf_batch(6, 5, 4)
    with pytest.raises(ValueError):
        fcd.crf_beam_search_nbest(xc[0], init[0], "NACGT", 6, beam_size=5)
    with pytest.raises(TypeError):
        fcd.crf_beam_search_nbest_batch_raw(xc, init, None, 5)
    # the C ABI refuses n_best outside 1 .. beam_size itself
    from fast_ctc_decode_amd import _native as nat
    import ctypes as C
    h = nat.default_handle()
    b = nat.Batch(x.ctypes.data, x.shape[0], x.shape[1], 1, 5, x.shape[1] * 5, 5, 0, 1, None)
    out = np.zeros((x.shape[0] * 6, x.shape[1]), np.uint8)
    ol = np.zeros(x.shape[0] * 6, np.uint32)
    st = np.zeros(x.shape[0], np.int32)
    sc = np.zeros(x.shape[0] * 6, np.float32)
    nh = np.zeros(x.shape[0], np.uint32)
    res = nat.Result(out.ctypes.data, None, None, ol.ctypes.data, st.ctypes.data, x.shape[1], None)
    for n_best in (0, 6, -1):
        nb = nat.NBest(n_best, sc.ctypes.data, nh.ctypes.data)
        assert h.lib.fcd_beam_search_nbest_host(h.ptr, C.byref(b), 5, 0.0, 1, 0, C.byref(nb), C.byref(res)) == nat.E_INVALID
    nb = nat.NBest(6, sc.ctypes.data, nh.ctypes.data)
    assert h.lib.fcd_beam_search_nbest_host(h.ptr, C.byref(b), 6, 0.0, 1, 0, C.byref(nb), C.byref(res)) == nat.OK
    assert (nh >= 1).sum() >= 5
