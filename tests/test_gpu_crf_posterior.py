"""-m gpu: the CRF substitution-posterior kernels (csrc/crf_posterior.hip) on the device.  The table of
tests/crf_posterior_cases.py and its cases outside the table (chains cut by the end, S = 1, the band against both cuts,
heavy variants, several workspace groups) on torch device tensors (fcd_crf_posterior_dev) against the restatement
(tests/crf_posterior_reference.py); the edge rows through _dev into poisoned outputs; 64 reads of the headline CRF shape cut
to 400 rows, decoded by crf_beam_search_batch_raw and scored at band 16; and the search -> posterior pipeline under
set_overlap(4) with no join in between."""
import ctypes as C
import math

import numpy as np
import pytest

import crf_lattice_cases as CC
import crf_posterior_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.fixture(scope="module")
def cases():
    by_name = {c[0]: c for c in PC.CASES}
    return {n: PC.build_case(by_name[n]) for n in PC.GPU_CASES}  # built once, shared, never changed


@pytest.mark.parametrize("name", PC.GPU_CASES)
def test_cases_on_device_tensors(fcd, cases, name):
    PC.run_case(fcd, cases[name], device="cuda")


@pytest.mark.parametrize("S,N", [(4, 5), (16, 5), (64, 5), (1024, 5), (8, 3), (8, 9)])
def test_chains_cut_by_the_end(fcd, S, N):
    PC.chains_cut_by_the_end(fcd, S, N, device="cuda")


def test_single_state_model(fcd):
    PC.single_state_model(fcd, device="cuda")


@pytest.mark.parametrize("band", [1, 4])
def test_band_against_both_cuts(fcd, band):
    PC.band_against_both_cuts(fcd, band, device="cuda")


def test_heavy_variants(fcd):
    PC.heavy_variants(fcd, device="cuda")


def test_workspace_limit_groups(fcd):
    PC.workspace_limit_groups(fcd, device="cuda")


def test_edge_rows_into_poisoned_outputs(fcd):
    """straight through fcd_crf_posterior_dev: every entry k < len is written, no other"""
    import torch
    from fast_ctc_decode_amd import _native as nat
    x, init, labels, lens, lengths = PC.edge_batch()
    dev = torch.device("cuda")
    xd, idv, ld, nd, td = (torch.from_numpy(a).to(dev) for a in (x, init, labels, lens.view(np.int32), lengths))
    post = torch.empty((12, 8, 4), dtype=torch.float32, device=dev).fill_(77.0)
    logp = torch.empty(12, dtype=torch.float64, device=dev).fill_(77.0)
    h = nat.default_handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    b = nat.Batch(xd.data_ptr(), 12, 6, 4, 5, 120, 20, 5, 1, td.data_ptr())
    y = nat.Labellings(ld.data_ptr(), nd.data_ptr(), None, None, 1, 8)
    out = nat.Posterior(post.data_ptr(), logp.data_ptr())
    assert h.lib.fcd_crf_posterior_dev(h.ptr, C.byref(b), C.c_void_p(idv.data_ptr()), 4, 4, C.byref(y), 0, C.byref(out)) == nat.OK
    torch.cuda.synchronize()
    PC.check_edges(post.cpu().numpy(), logp.cpu().numpy(), x, init, labels, lens, lengths, 77.0)


def test_headline_shape_decoded_then_scored(fcd):
    """64 reads of (T = 400, S = 4, N = 5), beam 5, 3-best: logp is crf_score's on every hypothesis, the posteriors at band 16
    are the restatement's on 4 reads' best hypotheses"""
    import torch
    rng = np.random.default_rng(21)
    x = CC.posteriors(rng, 64, 400, 4, 5)
    init = rng.random((64, 4)).astype(np.float32)
    xd, idv = torch.from_numpy(x).cuda(), torch.from_numpy(init).cuda()
    nb = fcd.crf_beam_search_nbest_batch_raw(xd, idv, 3, beam_size=5)
    got = nb.crf_posterior(xd, idv, band=16)
    score = nb.crf_score(xd, idv, band=16)
    torch.cuda.synchronize()
    assert got.post.shape == (64, 3, nb.labels.shape[2], 4)
    assert np.array_equal(got.logp.cpu().numpy(), score.cpu().numpy(), equal_nan=True)
    r, g = nb.cpu(), got.cpu()
    assert np.isfinite(g.logp[:, 0]).all()
    for b in (0, 21, 42, 63):
        n = int(r.out_len[b, 0])
        some = sorted(set(range(0, n, 13)) | {1, n - 2, n - 1})  # (the restatement takes a second per dozen positions here)
        pos, ref, lp = PC.reference_one(x[b], init[b], r.labels[b, 0, :n], 16, r.path[b, 0, :n], some)
        assert n > 50 and abs(g.logp[b, 0] - lp) <= CC.tolerance(400)
        PC.check_one(g.post[b, 0, pos], ref, 400, ("headline", b))
        conf = g.conf(r.labels)[b, 0, :n]
        assert (conf > 0).all() and (conf <= 1).all() and np.isfinite(g.post[b, 0, :n]).all()


def test_search_then_crf_posterior_under_overlap(fcd):
    """Four batches back to back: each search goes to an internal stream, each posterior call to the handle's stream,
    ordered by the library behind the searches in flight."""
    import torch
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(12)
    xs = [torch.from_numpy(CC.posteriors(rng, 32, 120, 4, 5)).cuda() for _ in range(4)]
    init = torch.from_numpy(rng.random((32, 4)).astype(np.float32)).cuda()
    h = nat.default_handle(0)

    def pipeline():
        out = []
        for x in xs:
            r = fcd.crf_beam_search_batch_raw(x, init, 8, 0.0)
            out.append((r, r.crf_posterior(x, init, band=16), r.crf_posterior(x, init)))
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
    x0, i0 = xs[0].cpu().numpy(), init.cpu().numpy()
    for got, band in zip(overlapped[0], (16, 0)):  # batch 0, two reads, both calls
        for b in (0, 17):
            n = int(rc.out_len[b])
            pos, ref, lp = PC.reference_one(x0[b], i0[b], rc.labels[b, :n], band, rc.path[b, :n] if band else None)
            assert math.isfinite(lp) and abs(got.logp[b, 0] - lp) <= CC.tolerance(120)
            PC.check_one(got.post[b, 0, pos], ref, 120, ("overlap", band, b))
