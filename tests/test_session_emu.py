"""CPU-side check of the beam-search sessions (include/fcd.h, fcd_beam_session_*; the SES instantiations of
csrc/beam_wave.hip and csrc/beam_generic.hip and the restart kernel of csrc/session.hip, compiled against tests/hipemu's
lockstep wave64 emulation): every kernel family a session runs on, plain and CRF, under both tie orders -- the result
after every push equals the oracle on each slot's prefix, the final one the one-shot call on the whole reads; failures,
restarts, refused pushes, f16 and time-major chunks.  The -m gpu twin is tests/test_gpu_session.py."""
import numpy as np
import pytest

import session_cases as SC
from emu_util import emulated_kernels
from tie_util import ORDERS, tie_order


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N,beam,kernel", SC.PLAIN)
def test_plain_every_push(fcd, order, N, beam, kernel):
    with tie_order(fcd, order):
        SC.run_plain(fcd, N, beam, kernel)


def test_plain_no_collapse_threshold(fcd):
    with tie_order(fcd, "pdq178"):
        SC.run_plain(fcd, 5, 5, SC.KERNEL_WAVE, seed=1, thr=0.05, collapse=False)
        SC.run_plain(fcd, 12, 5, SC.KERNEL_GENERIC, seed=1, thr=0.05, collapse=False)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N,S,beam,kernel", SC.CRF)
def test_crf_every_push(fcd, order, N, S, beam, kernel):
    with tie_order(fcd, order):
        SC.run_crf(fcd, N, S, beam, kernel)


@pytest.mark.parametrize("N,beam,kernel", [(5, 5, SC.KERNEL_WAVE), (12, 5, SC.KERNEL_GENERIC)])
def test_ran_out_of_beam(fcd, N, beam, kernel):
    SC.run_out_of_beam(fcd, N, beam, kernel)


@pytest.mark.parametrize("N,beam,kernel", [(5, 5, SC.KERNEL_WAVE), (7, 8, SC.KERNEL_WAVE1), (12, 5, SC.KERNEL_GENERIC)])
def test_restart(fcd, N, beam, kernel):
    SC.run_restart(fcd, N, beam, kernel)


@pytest.mark.parametrize("N,S,beam,kernel", SC.CRF)
def test_crf_restart(fcd, N, S, beam, kernel):
    SC.run_crf_restart(fcd, N, S, beam, kernel)


@pytest.mark.parametrize("N,beam,kernel", [(5, 5, SC.KERNEL_WAVE), (12, 5, SC.KERNEL_GENERIC)])
def test_over_long_push_refused(fcd, N, beam, kernel):
    SC.run_refused(fcd, N, beam, kernel)


@pytest.mark.parametrize("N,beam,kernel", [(5, 5, SC.KERNEL_WAVE), (12, 5, SC.KERNEL_GENERIC)])
def test_f16_and_time_major_chunks(fcd, N, beam, kernel):
    """f16 chunks (read exactly) and time-major (T, B, N) storage seen as a batch: the result of the upcast matrix"""
    x = SC.plain_batch(31, N).astype(np.float16)
    xf = x.astype(np.float32)
    B, T = x.shape[:2]
    with fcd.BeamSearchSession(B, N, T, beam, 0.0, kernel=kernel) as s:
        s.push(x[:, :17])
        tm = np.ascontiguousarray(xf[:, 17:].transpose(1, 0, 2)).transpose(1, 0, 2)  # float32, time-major strides
        assert tm.strides[1] > tm.strides[0]
        s.push(tm)
        r = s.result(host=True).cpu()
    for i in range(B):
        SC.check_slot(r, i, SC.want_plain(xf[i], beam, 0.0, True), "f16 / time-major")


def test_lane_kernel_refused_and_errors(fcd):
    with pytest.raises(RuntimeError, match="lane kernel"):
        fcd.BeamSearchSession(4, 5, 10, 32, kernel=SC.KERNEL_LANE)
    with pytest.raises(RuntimeError, match="wave kernel"):
        fcd.BeamSearchSession(4, 12, 10, 5, kernel=SC.KERNEL_WAVE)
    x = SC.plain_batch(1, 5)
    with fcd.BeamSearchSession(x.shape[0], 5, 60, 5) as s:
        with pytest.raises(ValueError):
            s.push(x[:3])  # n_reads differs
        with pytest.raises(ValueError):
            s.push(x, lengths=[1, 2])
        r = s.result(host=True).cpu()  # before any push: reads of length 0
        assert (np.asarray(r.status) == 0).all() and (np.asarray(r.out_len) == 0).all()
        assert s.nbytes > 0
        with pytest.raises(ValueError, match="twice"):
            s.restart([1, 2, 1])
        with pytest.raises(ValueError, match="range"):
            s.restart([6])


def test_sequences(fcd):
    x = SC.plain_batch(2, 5)
    B = x.shape[0]
    with fcd.BeamSearchSession(B, 5, 60, 5) as s:
        s.push(x[:, :30])
        s.push(x[:, 30:])
        seqs = s.result(host=True).sequences("NACGT", raise_on_error=False)
    for i in range(B):
        if i == 4:
            assert seqs[i] is None  # the NaN read
            continue
        assert seqs[i] == fcd.beam_search(x[i], "NACGT", 5)
    xc, init = SC.crf_batch(3, 5, 4)
    alpha = ["N", "AB", "C", "GT", "T"]
    with fcd.CrfBeamSearchSession(xc.shape[0], 4, 5, init, xc.shape[1], 5) as s:
        s.push(xc)
        seqs = s.result(host=True).sequences(alpha, raise_on_error=False)
    assert seqs[0] == fcd.crf_beam_search(xc[0], init[0], alpha, 5)
