"""-m gpu: the CRF lattice kernels (csrc/crf_lattice.hip) on the device.  A slice of the grid of
tests/test_crf_lattice_emu.py -- one case per K, both staging regimes, f16, time-major -- on torch device tensors
(fcd_crf_*_dev) and on numpy (fcd_crf_*_host) against the restatement (tests/crf_lattice_reference.py; what is compared and
how: tests/crf_lattice_cases.py); parity with crf_greedy_search on its own output; the edge cases; 64 reads of BASELINE
config 4's shape cut to 400 rows at S = 4, 64 and 1024, straight from the device search, at bands 16 and 64; and the
search -> align pipeline under set_overlap(4)."""
import math

import numpy as np
import pytest

import crf_lattice_cases as CC
from ctc_align_cases import host_abi_optional_pointers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.fixture(scope="module")
def cases():
    return {c[0]: CC.build_case(c) for c in CC.CASES if c[0] in CC.GPU_CASES}  # built once, shared, never changed


@pytest.mark.parametrize("name", CC.GPU_CASES)
def test_cases_on_device_tensors(fcd, cases, name):
    CC.run_case(fcd, cases[name], device="cuda")


@pytest.mark.parametrize("name", CC.GPU_CASES[:3])
def test_cases_on_numpy(fcd, cases, name):
    CC.run_case(fcd, cases[name])


@pytest.mark.parametrize("T", [65, 200])
def test_greedy_parity(fcd, T):
    CC.greedy_parity(fcd, T, "f16", device="cuda")
    CC.greedy_parity(fcd, T, "f32")


def test_host_abi_optional_pointers(fcd):
    host_abi_optional_pointers(fcd, S=4)


def test_edge_cases(fcd):
    import torch
    rng = np.random.default_rng(21)
    B, T, S, N = 8, 6, 4, 5
    x = CC.posteriors(rng, B, T, S, N)
    init = np.tile(np.array([0.1, 0.7, 0.7, 0.2], np.float32), (B, 1))
    labels = np.zeros((B, 8), np.uint8)
    lens = np.zeros(B, np.int32)
    lengths = np.full(B, 6, np.int64)
    # 0: L = 0   1: T_r = 0, L = 0   2: T_r = 0 < L   3: L > T_r   4: label N   5: a NaN that enters   6: L = T_r   7: len > stride
    lengths[1] = lengths[2] = 0
    labels[2, :1], lens[2] = [1], 1
    labels[3, :7], lens[3] = [1, 2, 1, 2, 1, 2, 1], 7
    labels[4, :2], lens[4] = [1, 5], 2
    labels[5, :2], lens[5] = [3, 1], 2  # sigma = 1, 2, 0
    x[5, 3, 2, 0] = np.nan
    labels[6, :6], lens[6] = [1, 2, 3, 4, 1, 2], 6
    labels[7, :], lens[7] = 1, 9
    dev = [torch.from_numpy(a).cuda() for a in (x, init, labels, lens, lengths)]
    got = fcd.crf_align_batch_raw(dev[0], dev[1], dev[2], dev[3], lengths=dev[4]).cpu()
    sc = fcd.crf_score_batch_raw(dev[0], dev[1], dev[2], dev[3], lengths=dev[4]).cpu().numpy()
    host = fcd.crf_align_batch_raw(x, init, labels, lens.astype(np.uint32), lengths=lengths)
    for name in ("start", "count", "qual", "logp"):
        assert np.array_equal(getattr(got, name), getattr(host, name), equal_nan=True), name
    lp = got.logp[:, 0]
    assert abs(lp[0] - np.log(x[0, :, 1, 0].astype(np.float64)).sum()) <= 6 * 2.0 ** -24 and abs(sc[0, 0] - lp[0]) <= 6 * 2.0 ** -24
    assert lp[1] == 0.0 and sc[1, 0] == 0.0
    assert lp[2] == lp[3] == -math.inf and sc[2, 0] == sc[3, 0] == -math.inf
    assert all(math.isnan(lp[b]) and math.isnan(sc[b, 0]) for b in (4, 5, 7))
    assert got.start[6, 0, :6].tolist() == list(range(6)) and (np.delete(got.count, 6, 0) == 0).all()
    CC.check(got, sc, x, init, lengths, labels[:, None, :], None, lens[:, None], None, 0, rows=[0, 1, 2, 3, 4, 5, 6])


@pytest.mark.parametrize("S", [4, 64, 1024])
def test_config4_shape(fcd, S):
    """64 reads x 400 rows x S x 5 in f16 (S = 4 is BASELINE config 4's shape cut to 400 rows; S = 1024 is gathered from
    global memory): the device search's own results, scored and aligned at bands 16 and 64, all 64 reads sane and every
    eighth (band 16) or sixteenth (band 64) against the restatement"""
    import torch
    B, T, N = 64, 400, 5
    rng = np.random.default_rng(30 + S)
    x = rng.random((B, T, S, N), dtype=np.float32)
    x[..., 0] *= 3.0
    x = (x / x.sum(-1, keepdims=True)).astype(np.float16)
    init = rng.random((B, S), dtype=np.float32)
    lengths = rng.integers(200, T + 1, size=B).astype(np.int64)
    lengths[0] = T
    xd = torch.from_numpy(x).cuda()
    r = fcd.crf_beam_search_batch_raw(xd, init, 5, 0.0, lengths=lengths)
    rc = r.cpu()
    assert (np.asarray(rc.status) == 0).all()
    for band, step in ((16, 8), (64, 16)):
        got = r.crf_align(xd, init, lengths=lengths, band=band)
        sc = r.crf_score(xd, init, lengths=lengths, band=band)
        assert got.logp.is_cuda and sc.is_cuda and tuple(sc.shape) == (B, 1)
        got, sc = got.cpu(), sc.cpu().numpy()
        assert np.isfinite(got.logp).all() and np.isfinite(sc).all() and (got.logp <= sc + CC.tolerance(T)).all()
        rows = range(0, B, step)
        x32 = np.zeros((B, T, S, N), np.float32)
        for b in rows:
            x32[b] = x[b].astype(np.float32)
        CC.check(got, sc, x32, init, lengths, rc.labels[:, None, :], rc.path[:, None, :], rc.out_len[:, None], None, band,
                 rows=rows)


def test_search_then_crf_align_under_overlap(fcd):
    """Four batches back to back: each search goes to an internal stream, each score / alignment to the handle's stream,
    ordered by the library behind the searches in flight -- no join in between; the joined run gives the same arrays."""
    import torch
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(12)
    xs = [torch.from_numpy(CC.posteriors(rng, 64, 300, 4, 5)).cuda() for _ in range(4)]
    init = torch.from_numpy(rng.random((64, 4), dtype=np.float32)).cuda()
    h = nat.default_handle(0)

    def pipeline():
        out = []
        for x in xs:
            r = fcd.crf_beam_search_batch_raw(x, init, 8, 0.0)
            out.append((r, r.crf_align(x, init, band=16), r.crf_align(x, init), r.crf_score(x, init, band=16)))
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        h.overlap_join()
        torch.cuda.synchronize()
        return [(a.cpu(), b.cpu(), s.cpu().numpy()) for _, a, b, s in out], out

    in_order, _ = pipeline()
    h.set_overlap(4)
    try:
        overlapped, keep = pipeline()
    finally:
        h.set_overlap(0)
    for t0, t1 in zip(in_order, overlapped):
        for a0, a1 in zip(t0[:2], t1[:2]):
            for name in ("start", "count", "qual", "logp"):
                assert np.array_equal(getattr(a0, name), getattr(a1, name), equal_nan=True), name
            assert np.isfinite(a0.logp[:, 0]).all()
        assert np.array_equal(t0[2], t1[2])
    rc = keep[0][0].cpu()
    x0 = xs[0].cpu().numpy()
    CC.check(overlapped[0][0], overlapped[0][2], x0, init.cpu().numpy(), None, rc.labels[:, None, :], rc.path[:, None, :],
             rc.out_len[:, None], None, 16, rows=range(0, 64, 8))
