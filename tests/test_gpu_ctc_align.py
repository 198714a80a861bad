"""-m gpu: the CTC forced-alignment kernels (csrc/ctc_align.hip) on the device.  The cases of tests/test_ctc_align_emu.py
on torch device tensors (fcd_ctc_align_dev) and on numpy (fcd_ctc_align_host) against the restatement
(tests/ctc_align_reference.py; what is compared and how: tests/ctc_align_cases.py); parity with viterbi_search on its own
output; BatchResult.ctc_align / NBestResult.ctc_align straight from device searches; one multi-tile case launched in
several groups (the workspace cap at a quarter of the need); and the search -> align pipeline under set_overlap(4)."""
import numpy as np
import pytest

import ctc_align_cases as AC
import ctc_score_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.fixture(scope="module")
def cases(fcd):
    return {c[0]: SC.build_case(fcd, c) for c in SC.CASES}  # built once, shared, never changed


@pytest.mark.parametrize("name", [c[0] for c in SC.CASES])
def test_cases_on_device_tensors(fcd, cases, name):
    AC.run_case(fcd, cases[name], device="cuda")


@pytest.mark.parametrize("name", [c[0] for c in SC.CASES])
def test_cases_on_numpy(fcd, cases, name):
    AC.run_case(fcd, cases[name])


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("T", [1, 65, 200])
def test_greedy_parity(fcd, T, dtype):
    AC.greedy_parity(fcd, T, dtype, device="cuda")
    AC.greedy_parity(fcd, T, dtype)


def test_host_abi_optional_pointers(fcd):
    AC.host_abi_optional_pointers(fcd)


def test_results_align_themselves_on_the_device(fcd):
    import torch
    rng = np.random.default_rng(11)
    x = SC.posteriors(rng, 16, 200, 5)
    lengths = rng.integers(100, 201, size=16).astype(np.int64)
    xd = torch.from_numpy(x).cuda()
    r = fcd.beam_search_batch_raw(xd, 5, 0.0, lengths=lengths)
    rc = r.cpu()
    for band in (16, 0):
        got = r.ctc_align(xd, lengths=lengths, band=band)
        assert all(a.is_cuda for a in (got.start, got.count, got.qual, got.logp))
        assert got.logp.dtype == torch.float64 and tuple(got.logp.shape) == (16, 1) and tuple(got.start.shape) == (16, 1, 200)
        AC.check(got.cpu(), x, lengths, rc.labels[:, None, :], rc.path[:, None, :], rc.out_len[:, None], None, True, band)
    nb = fcd.beam_search_nbest_batch_raw(xd, 5, beam_size=8, beam_cut_threshold=0.02, lengths=lengths)
    nc = nb.cpu()
    for band in (16, 0):
        got = nb.ctc_align(xd, lengths=lengths, band=band)
        assert got.qual.is_cuda and tuple(got.qual.shape) == (16, 5, 200)
        AC.check(got.cpu(), x, lengths, nc.labels, nc.path, nc.out_len, nc.n_hyp, True, band)


def test_multi_tile_in_groups(fcd):
    """64 reads of 1000 rows at band 16 (16 tiles of 64 rows each, 64 KB of back-pointers a read) with the workspace cap at a
    quarter of the need: four launches, the same result as one, and the restatement's on 8 reads"""
    import torch
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(13)
    x = SC.posteriors(rng, 64, 1000, 5)
    lengths = rng.integers(500, 1001, size=64).astype(np.int64)
    lengths[0] = 1000
    xd = torch.from_numpy(x).cuda()
    h = nat.Handle(0)
    r = fcd.beam_search_batch_raw(xd, 5, 0.0, lengths=lengths, handle=h)
    whole = r.ctc_align(xd, lengths=lengths, band=16).cpu()
    h.set_align_workspace_cap(64 * 1000 * 64 // 4)
    parts = r.ctc_align(xd, lengths=lengths, band=16).cpu()
    h.set_align_workspace_cap(0)
    for name in ("start", "count", "qual", "logp"):
        assert np.array_equal(getattr(whole, name), getattr(parts, name), equal_nan=True), name
    rc = r.cpu()
    AC.check(parts, x, lengths, rc.labels[:, None, :], rc.path[:, None, :], rc.out_len[:, None], None, True, 16,
             rows=range(0, 64, 8))
    h.close()


def test_search_then_align_under_overlap(fcd):
    """Four batches back to back: each search goes to an internal stream, each alignment to the handle's stream, ordered
    by the library behind the searches in flight."""
    import torch
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(12)
    xs = [torch.from_numpy(SC.posteriors(rng, 64, 300, 5)).cuda() for _ in range(4)]
    h = nat.Handle(0)

    def pipeline():
        out = []
        for x in xs:
            r = fcd.beam_search_batch_raw(x, 8, 0.0, handle=h)
            out.append((r, r.ctc_align(x, band=16), r.ctc_align(x)))
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
            for name in ("start", "count", "qual", "logp"):
                assert np.array_equal(getattr(a0, name), getattr(a1, name), equal_nan=True), name
            assert np.isfinite(a0.logp[:, 0]).all()
    rc = keep[0][0].cpu()
    x0 = xs[0].cpu().numpy()
    for got, band in zip(overlapped[0], (16, 0)):  # batch 0, every read, both calls
        AC.check(got, x0, None, rc.labels[:, None, :], rc.path[:, None, :], rc.out_len[:, None], None, True, band)
    h.close()


def test_lds_window_beyond_sixteen_cells_per_work_item(fcd):
    AC.wide_window_parity(fcd)


def test_beam_search_qstring_falls_back_to_a_band(fcd):
    """9500 rows and as many possible labels: the exact lattice (19001 states) does not fit the LDS, so the quality
    string comes from band 64 around the search's path"""
    rng = np.random.default_rng(14)
    x = SC.posteriors(rng, 1, 9500, 5)[0]
    seq, path = fcd.beam_search(x, "NACGT", 5, 0.0)
    n = len(seq)
    lab = np.zeros((1, 9500), np.uint8)
    lab[0, :n] = ["NACGT".index(c) for c in seq]
    pth = np.zeros((1, 9500), np.uint32)
    pth[0, :n] = path
    with pytest.raises(fcd._native.NativeError) as e:
        fcd.ctc_align_batch_raw(x[None], lab, [n])
    assert e.value.code == fcd._native.E_UNSUPPORTED
    want = fcd.ctc_align_batch_raw(x[None], lab, [n], paths=pth, band=64).qstrings(np.array([[n]]))[0][0]
    got, got_path = fcd.beam_search(x, "NACGT", 5, 0.0, qstring=True)
    assert got_path == path and got == seq + want and len(want) == n
