"""Beam-search sessions on the MI355X (include/fcd.h, fcd_beam_session_*): the case matrix of tests/session_cases.py with
torch device chunks and device results (every push against the oracle on each slot's prefix, the final result against
the one-shot call), BASELINE config 2 at full size pushed as 10 x 400 rows and as 7 uneven chunks under both tie orders,
config 4's CRF shape, 64 reads of each against the oracle at 3 intermediate prefixes, and a session pushed while
overlapping one-shot calls are in flight.  The CPU twin is tests/test_session_emu.py."""
import numpy as np
import pytest

import session_cases as SC
import test_gpu_parity as P
from tie_util import ORDERS, tie_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def dev(torch):
    def to(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return to


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N,beam,kernel", SC.PLAIN)
def test_plain_every_push(fcd, torch, order, N, beam, kernel):
    with tie_order(fcd, order):
        SC.run_plain(fcd, N, beam, kernel, to_input=dev(torch), host=False)


def test_plain_no_collapse_threshold(fcd, torch):
    SC.run_plain(fcd, 5, 5, SC.KERNEL_WAVE, seed=1, thr=0.05, collapse=False, to_input=dev(torch), host=False)
    SC.run_plain(fcd, 12, 5, SC.KERNEL_GENERIC, seed=1, thr=0.05, collapse=False, to_input=dev(torch), host=False)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N,S,beam,kernel", SC.CRF)
def test_crf_every_push(fcd, torch, order, N, S, beam, kernel):
    with tie_order(fcd, order):
        SC.run_crf(fcd, N, S, beam, kernel, to_input=dev(torch), host=False)


@pytest.mark.parametrize("N,beam,kernel", [(5, 5, SC.KERNEL_WAVE), (12, 5, SC.KERNEL_GENERIC)])
def test_failures_restarts_refusals(fcd, torch, N, beam, kernel):
    SC.run_out_of_beam(fcd, N, beam, kernel, host=False)
    SC.run_restart(fcd, N, beam, kernel, host=False)
    SC.run_refused(fcd, N, beam, kernel, host=False)


@pytest.mark.parametrize("N,S,beam,kernel", SC.CRF)
def test_crf_restart(fcd, torch, N, S, beam, kernel):
    SC.run_crf_restart(fcd, N, S, beam, kernel, host=False)


@pytest.mark.parametrize("N,beam,kernel", [(5, 5, SC.KERNEL_AUTO), (7, 8, SC.KERNEL_WAVE1), (12, 5, SC.KERNEL_GENERIC)])
def test_f16_time_major_device_chunks(fcd, torch, N, beam, kernel):
    x = SC.plain_batch(31, N).astype(np.float16)
    xf = x.astype(np.float32)
    B, T = x.shape[:2]
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).cuda().transpose(0, 1)  # (T, B, N) storage
    with fcd.BeamSearchSession(B, N, T, beam, 0.0, kernel=kernel) as s:
        s.push(xt[:, :17])
        r = s.push(xt[:, 17:].float(), result=True).cpu()  # the dtype may change from push to push
    for i in range(B):
        SC.check_slot(r, i, SC.want_plain(xf[i], beam, 0.0, True) + (), "f16 / time-major")


UNEVEN = [0, 1, 400, 1400, 1403, 3000, 3600, 4000]  # 7 chunks


def _oracle_reads(x_host_fn, idx, prefix, r, want_fn):
    for i in idx:
        SC.check_slot(r, int(i), want_fn(x_host_fn(int(i), prefix)), "prefix %d" % prefix)


@pytest.mark.parametrize("order", ORDERS)
def test_config2_full_size(fcd, torch, order):
    """4096 x 4000 x 5, beam 5, threshold 0.1: 10 x 400-row pushes and 7 uneven ones equal the one-shot call read for
    read; 64 reads against the oracle after the pushes that end at rows 400, 1403 and 3000"""
    B, T = 4096, 4000
    x = P.gen_batch(2024, B, T, 5)
    xd = dev(torch)(x)
    idx = np.linspace(0, B - 1, 64).astype(int)
    with tie_order(fcd, order):
        one = fcd.beam_search_batch_raw(xd, 5, 0.1).cpu()
        for bounds in (list(range(0, T + 1, 400)), UNEVEN):
            with fcd.BeamSearchSession(B, 5, T, 5, 0.1) as s:
                for a, b in zip(bounds[:-1], bounds[1:]):
                    r = s.push(xd[:, a:b], result=b in (400, 1403, 3000))
                    if r is not None and bounds is UNEVEN:
                        r = r.cpu()
                        for i in idx:
                            st, labels, path, _ = SC.oracle.beam_search_ambiguous(np.ascontiguousarray(x[i, :b]), 5, 0.1)
                            SC.check_slot(r, int(i), (st, labels, path, None), "prefix %d" % b)
                final = s.result().cpu()
            SC.same_result(final, one, "config 2, chunks %s" % bounds[:3])
    assert (np.asarray(one.status) == 0).all()


def test_config4_crf_shape(fcd, torch):
    """4096 x 4000 x 4 states x 5, beam 5, one-hot init: 10 x 400-row pushes equal the one-shot call; 64 reads against
    the oracle at rows 400, 1400 and 3000"""
    B, T, S = 4096, 4000, 4
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    xd = torch.rand((B, T, S, 5), generator=g, device="cuda")
    xd /= xd.sum(-1, keepdim=True)
    init = torch.zeros((B, S), device="cuda")
    init[torch.arange(B), torch.arange(B) % S] = 1.0
    idx = np.linspace(0, B - 1, 64).astype(int)
    xs = xd[torch.from_numpy(idx).cuda()].cpu().numpy()
    ini = init.cpu().numpy()
    one = fcd.crf_beam_search_batch_raw(xd, init, 5, 0.0).cpu()
    with fcd.CrfBeamSearchSession(B, S, 5, init, T, 5, 0.0) as s:
        for a in range(0, T, 400):
            r = s.push(xd[:, a:a + 400], result=a + 400 in (400, 1200, 3200))
            if r is not None:
                r = r.cpu()
                for j, i in enumerate(idx):
                    SC.check_slot(r, int(i), SC.want_crf(xs[j, :a + 400], ini[i], 5, 0.0)[:3] + (None,), "prefix %d" % (a + 400))
        final = s.result().cpu()
    SC.same_result(final, one, "config 4")
    assert (np.asarray(one.status) == 0).all()


def test_session_under_overlap(fcd, torch):
    """a session pushed between set_overlap(4) one-shot calls on the same handle: both results equal their stream-order
    runs"""
    xs = [dev(torch)(P.gen_batch(400 + i, 48, 500, 5)) for i in range(3)]
    y = dev(torch)(P.gen_batch(77, 64, 300, 5))

    def run():
        outs = []
        with fcd.BeamSearchSession(64, 5, 300, 5, 0.05) as s:
            for i, x in enumerate(xs):
                outs.append(fcd.beam_search_batch_raw(x, 32, 0.05, kernel=SC.KERNEL_LANE))
                s.push(y[:, 100 * i:100 * (i + 1)])
                outs.append(fcd.beam_search_batch_raw(x, 5, 0.05))
                mid = s.result()
            return [o.cpu() for o in outs], mid.cpu()

    want, want_s = run()
    fcd.set_overlap(4)
    try:
        got, got_s = run()
    finally:
        fcd.set_overlap(0)
    for a, b in zip(got, want):
        SC.same_result(a, b, "overlapping one-shot call")
    SC.same_result(got_s, want_s, "session")
    one = fcd.beam_search_batch_raw(y, 5, 0.05).cpu()
    SC.same_result(got_s, one, "session vs one-shot")
