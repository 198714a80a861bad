"""The n best hypotheses of the beam searches on the MI355X (include/fcd.h, fcd_nbest): every kernel family, plain and
CRF, under both tie orders, against tests/nbest_reference.py (labels, paths, bit-exact scores, n_hyp) with hypothesis 0
equal to the single-result call; f16 time-major device input; uninitialised (torch.empty) outputs; the wide-beam
two-pass retry; overlapping calls; and BASELINE configs 2 and 3 at full size."""
import numpy as np
import pytest

import nbest_cases as NC
import nbest_reference as NR
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


def poison_allocator(torch):
    """fill the caching allocator's free blocks with 0xFF, so that torch.empty outputs start as garbage"""
    t = torch.full((64 << 20,), 255, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    del t


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N,beam,kernel", NC.PLAIN)
def test_plain_every_family(fcd, torch, order, N, beam, kernel):
    poison_allocator(torch)
    with tie_order(fcd, order):
        NC.run_plain(fcd, N, beam, kernel, stable=order == "stable", to_input=dev(torch))
        NC.run_plain(fcd, N, beam, kernel, stable=order == "stable", thr=0.1, n_best=max(1, beam // 2), seed=1)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N,S,beam,kernel", NC.CRF)
def test_crf_every_family(fcd, torch, order, N, S, beam, kernel):
    poison_allocator(torch)
    with tie_order(fcd, order):
        NC.run_crf(fcd, N, S, beam, kernel, stable=order == "stable", to_input=dev(torch))
        NC.run_crf(fcd, N, S, beam, kernel, stable=order == "stable", n_best=1, seed=1)


@pytest.mark.parametrize("N,beam,kernel", [(5, 5, NC.KERNEL_WAVE), (5, 32, NC.KERNEL_LANE), (12, 5, NC.KERNEL_GENERIC)])
def test_ran_out_of_beam(fcd, N, beam, kernel):
    NC.run_out_of_beam(fcd, N, beam, kernel)


@pytest.mark.parametrize("N,beam,kernel", [(5, 5, NC.KERNEL_AUTO), (5, 32, NC.KERNEL_LANE), (7, 8, NC.KERNEL_GENERIC)])
def test_f16_time_major(fcd, torch, N, beam, kernel):
    x, lengths = NC.plain_batch(31 + beam, N)
    x = x.astype(np.float16).astype(np.float32)  # what the kernels read, exactly
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2)).astype(np.float16)).cuda().transpose(0, 1)
    assert xt.stride(1) == x.shape[0] * N  # (T, B, N) storage seen as a (B, T, N) batch
    r = fcd.beam_search_nbest_batch_raw(xt, beam, beam, 0.0, lengths=lengths, kernel=kernel).cpu()
    want = [NR.beam_search(x[i, :lengths[i]], beam, 0.0) for i in range(x.shape[0])]
    NC.check(r, want, beam, x.shape[0])
    NC.check_hyp0(r, fcd.beam_search_batch_raw(xt, beam, 0.0, lengths=lengths, kernel=kernel).cpu(), x.shape[0])


def test_lane_two_pass_retry(fcd, torch):
    """a small workspace limit and a large first-pass divisor: most reads overflow their first-pass slab and are decoded
    again by the retry pass, which must rewrite all n_best rows of each"""
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(3)
    B, T = 11, 300
    x = rng.random((B, T, 5), dtype=np.float32)
    x /= x.sum(-1, keepdims=True)
    x[3] = 0.2
    x[7, 150] = np.nan
    lengths = np.array([T, T, 1, T, 0, T, 299, T, T, 64, T], np.int64)
    h = nat.default_handle()
    h.set_workspace_limit(2 << 20)
    h.check(h.lib.fcd_debug_set_first_pass_divisor(h.ptr, 6))
    try:
        for beam, n_best in ((32, 32), (20, 7)):
            poison_allocator(torch)
            r = fcd.beam_search_nbest_batch_raw(dev(torch)(x), n_best, beam, 0.0, lengths=lengths,
                                                kernel=fcd.KERNEL_LANE).cpu()
            want = [NR.beam_search(x[i, :lengths[i]], beam, 0.0) for i in range(B)]
            NC.check(r, want, n_best, B)
            NC.check_hyp0(r, fcd.beam_search_batch_raw(x, beam, 0.0, lengths=lengths, kernel=fcd.KERNEL_LANE), B)
    finally:
        h.check(h.lib.fcd_debug_set_first_pass_divisor(h.ptr, 0))
        h.set_workspace_limit(0)


def test_overlapping_calls(fcd, torch):
    """set_overlap(4): n-best calls interleaved with plain beam calls equal the same calls in stream order"""
    xs = [dev(torch)(P.gen_batch(400 + i, 48, 500, 5)) for i in range(3)]

    def calls():
        out = []
        for i, x in enumerate(xs):
            for beam, kernel in ((5, 0), (32, 4)):
                out.append(fcd.beam_search_nbest_batch_raw(x, 1 + i % 3, beam, 0.05, kernel=kernel))
                out.append(fcd.beam_search_batch_raw(x, beam, 0.05, kernel=kernel))
        return [r.cpu() for r in out]

    want = calls()
    fcd.set_overlap(4)
    try:
        got = calls()
    finally:
        fcd.set_overlap(0)
    for a, b in zip(got, want):
        for name in ("labels", "path", "out_len", "status", "score", "n_hyp"):
            if hasattr(b, name):
                assert np.array_equal(getattr(a, name), getattr(b, name)), name


def full_size(fcd, torch, B, beam, kernel, n_ref):
    x = P.gen_batch(2024, B, 4000, 5)
    xd = dev(torch)(x)
    r = fcd.beam_search_nbest_batch_raw(xd, beam, beam, 0.1, kernel=kernel).cpu()
    single = fcd.beam_search_batch_raw(xd, beam, 0.1, kernel=kernel).cpu()
    NC.check_hyp0(r, single, B)
    assert (r.status == 0).all() and (r.n_hyp == beam).all()
    assert (r.score[:, 1:] <= r.score[:, :-1]).all()  # rank order
    idx = np.linspace(0, B - 1, n_ref).astype(int)
    want = [NR.beam_search(x[i], beam, 0.1) for i in idx]
    sub = fcd.NBestResult(r.labels[idx], r.path[idx], r.out_len[idx], r.score[idx], r.n_hyp[idx], r.status[idx])
    NC.check(sub, want, beam, n_ref)


def test_baseline_config2(fcd, torch):
    """4096 x 4000 x 5, beam 5, threshold 0.1, n_best 5"""
    full_size(fcd, torch, 4096, 5, NC.KERNEL_AUTO, 16)


def test_baseline_config3_shape(fcd, torch):
    """beam 32 on the lane kernel, 256 reads of 4000 rows"""
    full_size(fcd, torch, 256, 32, NC.KERNEL_LANE, 8)
