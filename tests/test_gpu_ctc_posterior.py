"""-m gpu: the substitution-posterior kernels (csrc/ctc_posterior.hip) on the device.  The cases of
tests/ctc_posterior_cases.py on torch device tensors (fcd_ctc_posterior_dev) and on numpy (fcd_ctc_posterior_host) against
the restatement (tests/ctc_posterior_reference.py); the edge rows through _dev into uninitialised outputs; and the
search -> posterior pipeline under set_overlap(4) with no join in between."""
import ctypes as C

import numpy as np
import pytest

import ctc_posterior_cases as PC
import ctc_posterior_reference as PR
import ctc_score_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.fixture(scope="module")
def cases(fcd):
    return {c[0]: PC.build_case(fcd, c) for c in PC.CASES}  # built once, shared, never changed


@pytest.mark.parametrize("name", [c[0] for c in PC.CASES])
def test_cases_on_device_tensors(fcd, cases, name):
    PC.run_case(fcd, cases[name], device="cuda")


@pytest.mark.parametrize("name", [c[0] for c in PC.CASES])
def test_cases_on_numpy(fcd, cases, name):
    PC.run_case(fcd, cases[name])


def test_edge_rows_into_uninitialised_outputs(fcd):
    """straight through fcd_ctc_posterior_dev: outputs from torch.empty, poisoned -- every entry k < len is written, no
    other"""
    import torch
    from fast_ctc_decode_amd import _native as nat
    x, labels, lens, lengths = PC.edge_batch()
    dev = torch.device("cuda")
    xd, ld, nd, td = (torch.from_numpy(a).to(dev) for a in (x, labels, lens.view(np.int32), lengths))
    post = torch.empty((10, 8, 3), dtype=torch.float32, device=dev).fill_(77.0)
    logp = torch.empty(10, dtype=torch.float64, device=dev).fill_(77.0)
    h = nat.default_handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    b = nat.Batch(xd.data_ptr(), 10, 6, 1, 4, 24, 4, 0, 1, td.data_ptr())
    y = nat.Labellings(ld.data_ptr(), nd.data_ptr(), None, None, 1, 8)
    out = nat.Posterior(post.data_ptr(), logp.data_ptr())
    assert h.lib.fcd_ctc_posterior_dev(h.ptr, C.byref(b), C.byref(y), 1, 0, C.byref(out)) == nat.OK
    torch.cuda.synchronize()
    PC.check_edges(post.cpu().numpy(), logp.cpu().numpy(), x, labels, lens, lengths, 77.0)


def test_search_then_posterior_under_overlap(fcd):
    """Four batches back to back: each search goes to an internal stream, each posterior call to the handle's stream,
    ordered by the library behind the searches in flight."""
    import torch
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(12)
    xs = [torch.from_numpy(SC.posteriors(rng, 32, 120, 5)).cuda() for _ in range(4)]
    h = nat.Handle(0)

    def pipeline():
        out = []
        for x in xs:
            r = fcd.beam_search_batch_raw(x, 8, 0.0, handle=h)
            out.append((r, r.ctc_posterior(x, band=16), r.ctc_posterior(x)))
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        h.overlap_join()
        torch.cuda.synchronize()
        return [(a.cpu(), b.cpu()) for _, a, b in out], out

    in_order, _ = pipeline()
    h.set_overlap(4)
    try:
        overlapped, keep = pipeline()
    finally:
        h.set_overlap(0)
    for pair0, pair1 in zip(in_order, overlapped):
        for a0, a1 in zip(pair0, pair1):
            assert np.array_equal(a0.post, a1.post, equal_nan=True) and np.array_equal(a0.logp, a1.logp)
            assert np.isfinite(a0.logp).all()
    rc = keep[0][0].cpu()
    x0 = xs[0].cpu().numpy()
    for got, band in zip(overlapped[0], (16, 0)):  # batch 0, four reads, both calls
        for b in range(0, 32, 8):
            n = int(rc.out_len[b])
            ref, lp = PR.ctc_posterior(x0[b], rc.labels[b, :n], True, band, rc.path[b, :n] if band else None)
            assert SC.same(got.logp[b, 0], lp, 120)
            PC.check_one(got.post[b, 0, :n], ref, 120, ("overlap", band, b))
    h.close()
