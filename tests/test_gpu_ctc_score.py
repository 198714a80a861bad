"""-m gpu: the CTC forward scoring kernels (csrc/ctc_score.hip) on the device.  The cases of tests/test_ctc_score_emu.py
on torch device tensors (fcd_ctc_score_dev) and on numpy (fcd_ctc_score_host) against the float64 restatement
(tests/ctc_score_reference.py; tolerance and input condition: tests/ctc_score_cases.py); BASELINE config 2 at full size
(4096 x 4000 x 5, beam 5, threshold 0.1): the search on the device, hypothesis 0 of all 4096 reads scored at band 64
(256 reads checked) and in exact mode (32 reads checked); and the search -> score pipeline under set_overlap(4), four
batches back to back, whose scores must equal those of the same calls in stream order."""
import numpy as np
import pytest

import ctc_score_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("case", SC.CASES, ids=[c[0] for c in SC.CASES])
def test_cases_on_device_tensors(fcd, case):
    SC.run_case(fcd, SC.build_case(fcd, case), device="cuda", verbose=True)


@pytest.mark.parametrize("case", SC.CASES, ids=[c[0] for c in SC.CASES])
def test_cases_on_numpy(fcd, case):
    SC.run_case(fcd, SC.build_case(fcd, case), verbose=True)


def test_results_score_themselves_on_the_device(fcd):
    import torch
    rng = np.random.default_rng(11)
    x = SC.posteriors(rng, 16, 200, 5)
    lengths = rng.integers(100, 201, size=16).astype(np.int64)
    xd = torch.from_numpy(x).cuda()
    r = fcd.beam_search_batch_raw(xd, 5, 0.0, lengths=lengths)
    got = r.ctc_score(xd, lengths=lengths, band=16)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (16, 1)
    rc = r.cpu()
    SC.check(got.cpu().numpy(), x, lengths, rc.labels[:, None, :], rc.path[:, None, :], rc.out_len[:, None], None, True, 16)
    nb = fcd.beam_search_nbest_batch_raw(xd, 5, beam_size=8, beam_cut_threshold=0.02, lengths=lengths)
    got = nb.ctc_score(xd, lengths=lengths)
    nc = nb.cpu()
    SC.check(got.cpu().numpy(), x, lengths, nc.labels, nc.path, nc.out_len, nc.n_hyp, True, 0)


def test_config2_full_size(fcd):
    import torch
    from test_gpu_parity import gen_batch
    x = gen_batch(2024, 4096, 4000, 5)
    xd = torch.from_numpy(x).cuda()
    r = fcd.beam_search_batch_raw(xd, 5, 0.1)
    banded = r.ctc_score(xd, band=64)
    exact = r.ctc_score(xd)
    torch.cuda.synchronize()
    rc = r.cpu()
    assert (np.asarray(rc.status) == 0).all()
    banded, exact = banded.cpu().numpy(), exact.cpu().numpy()
    assert banded.shape == (4096, 1) and np.isfinite(banded).all() and np.isfinite(exact).all()
    labels, paths, out_len = rc.labels[:, None, :], rc.path[:, None, :], rc.out_len[:, None]
    SC.check(banded, x, None, labels, paths, out_len, None, True, 64, rows=range(0, 4096, 16), verbose=True)
    SC.check(exact, x, None, labels, paths, out_len, None, True, 0, rows=range(5, 4096, 128), verbose=True)
    assert (banded <= exact + 2 * SC.tolerance(4000)).all()  # the band is a lower bound, for every read


def test_search_then_score_under_overlap(fcd):
    """Four batches back to back: each search goes to an internal stream, each scoring call to the handle's stream,
    ordered by the library behind the search in flight that still writes the labels it reads."""
    import torch
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(12)
    xs = [torch.from_numpy(SC.posteriors(rng, 512, 600, 5)).cuda() for _ in range(4)]
    h = nat.Handle(0)

    def pipeline():
        out = []
        for x in xs:
            nb = fcd.beam_search_nbest_batch_raw(x, 3, beam_size=24, beam_cut_threshold=0.0, handle=h)
            out.append((nb, nb.ctc_score(x, band=16), nb.ctc_score(x)))
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        h.overlap_join()
        torch.cuda.synchronize()
        return [(a.cpu().numpy(), b.cpu().numpy()) for _, a, b in out], out

    in_order, _ = pipeline()
    h.set_overlap(4)
    try:
        overlapped, keep = pipeline()
    finally:
        h.set_overlap(0)
    for (a0, b0), (a1, b1) in zip(in_order, overlapped):
        assert np.array_equal(a0, a1, equal_nan=True) and np.array_equal(b0, b1, equal_nan=True)
        assert np.isfinite(b0[:, 0]).all()
    # and they are the right numbers
    nb = keep[0][0].cpu()
    SC.check(overlapped[0][1], xs[0].cpu().numpy(), None, nb.labels, nb.path, nb.out_len, nb.n_hyp, True, 0, rows=range(0, 512, 64))
    h.close()
