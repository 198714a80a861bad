"""-m gpu: the CRF deletion and insertion walks (csrc/crf_posterior.hip) on the device.  The table of
tests/crf_edits_cases.py on torch device tensors (fcd_crf_edits_dev) against the restatements
(tests/crf_edits_reference.py; the variants rescored one by one are the emulator file's share of the work), the edge rows
through _dev into poisoned outputs, heavy variants, EditResult.best's pick against crf_score, host and device entry points
side by side, several workspace groups, and the search -> edits pipeline under set_overlap(4) with no join in between."""
import ctypes as C
import math

import numpy as np
import pytest

import crf_edits_cases as EC
import crf_lattice_cases as CC
import crf_posterior_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.fixture(scope="module")
def cases():
    by_name = {c[0]: c for c in EC.CASES}
    return {n: EC.build_case(by_name[n]) for n in EC.GPU_CASES}  # built once, shared, never changed


@pytest.mark.parametrize("name", EC.GPU_CASES)
def test_cases_on_device_tensors(fcd, cases, name):
    EC.run_case(fcd, cases[name], device="cuda", rescore=False)


def test_edge_rows(fcd):
    EC.edge_rows(fcd, device="cuda")


def test_heavy_variants(fcd):
    EC.heavy_variants(fcd, device="cuda")


def test_best_edit_is_crf_score(fcd):
    EC.best_edit_is_crf_score(fcd, device="cuda")


def test_workspace_limit_groups(fcd):
    EC.workspace_limit_groups(fcd, device="cuda")


def test_host_and_device_entry_points_agree(fcd, cases):
    c = cases["m3_s64n5_t40_tm"]
    xin, conv, kw = CC._device_inputs(c, "cuda")
    for band in (0, 4):
        dev = fcd.crf_edits_batch_raw(xin, conv(c["init"]), conv(c["labels"]), conv(c["out_len"]), conv(c["lengths"]),
                                      conv(c["paths"]) if band else None, band, conv(c["n_valid"]), **kw).cpu()
        host = fcd.crf_edits_batch_raw(c["xin"], c["init"], c["labels"], c["out_len"], c["lengths"],
                                       c["paths"] if band else None, band, c["n_valid"])
        assert np.array_equal(dev.deletion, host.deletion, equal_nan=True)
        assert np.array_equal(dev.insertion, host.insertion, equal_nan=True)
        assert np.array_equal(dev.logp, host.logp, equal_nan=True)


def test_edge_rows_into_poisoned_outputs(fcd):
    """straight through fcd_crf_edits_dev: every entry k < len, g <= len is written, no other"""
    import torch
    from fast_ctc_decode_amd import _native as nat
    x, init, labels, lens, lengths = PC.edge_batch()
    dev = torch.device("cuda")
    xd, idv, ld, nd, td = (torch.from_numpy(a).to(dev) for a in (x, init, labels, lens.view(np.int32), lengths))
    dele = torch.empty((12, 8), dtype=torch.float32, device=dev).fill_(77.0)
    ins = torch.empty((12, 9, 4), dtype=torch.float32, device=dev).fill_(77.0)
    logp = torch.empty(12, dtype=torch.float64, device=dev).fill_(77.0)
    h = nat.default_handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    b = nat.Batch(xd.data_ptr(), 12, 6, 4, 5, 120, 20, 5, 1, td.data_ptr())
    y = nat.Labellings(ld.data_ptr(), nd.data_ptr(), None, None, 1, 8)
    out = nat.Edits(dele.data_ptr(), ins.data_ptr(), logp.data_ptr())
    assert h.lib.fcd_crf_edits_dev(h.ptr, C.byref(b), C.c_void_p(idv.data_ptr()), 4, 4, C.byref(y), 0, C.byref(out)) == nat.OK
    torch.cuda.synchronize()
    dele, ins, logp = dele.cpu().numpy(), ins.cpu().numpy(), logp.cpu().numpy()
    want = EC.edits(fcd, "cuda", x, init, labels, lens, lengths)
    assert np.array_equal(logp, want.logp[:, 0], equal_nan=True)
    for r in range(12):
        n = min(int(lens[r]), 8)
        assert np.array_equal(dele[r, :n], want.deletion[r, 0, :n], equal_nan=True) and (dele[r, n:] == 77).all(), r
        assert np.array_equal(ins[r, :n + 1], want.insertion[r, 0, :n + 1], equal_nan=True) and (ins[r, n + 1:] == 77).all(), r


def test_search_then_crf_edits_under_overlap(fcd):
    """Four batches back to back: each search goes to an internal stream, each edits call to the handle's stream, ordered by
    the library behind the searches in flight."""
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
            out.append((r, r.crf_edits(x, init, band=16), r.crf_edits(x, init)))
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
            assert np.array_equal(a0.deletion, a1.deletion, equal_nan=True) and np.array_equal(a0.insertion, a1.insertion, equal_nan=True)
            assert np.array_equal(a0.logp, a1.logp) and np.isfinite(a0.logp).all()
    rc = keep[0][0].cpu()
    x0, i0 = xs[0].cpu().numpy(), init.cpu().numpy()
    for got, band in zip(overlapped[0], (16, 0)):  # batch 0, two reads, both calls
        for b in (0, 17):
            n = int(rc.out_len[b])
            ref = EC.reference_one(x0[b], i0[b], rc.labels[b, :n], band, rc.path[b, :n] if band else None, rescore=False)
            assert math.isfinite(ref["chain"][2]) and abs(got.logp[b, 0] - ref["chain"][2]) <= CC.tolerance(120)
            EC.check_one(got.deletion[b, 0, :n], got.insertion[b, 0, :n + 1], ref, 120, ("overlap", band, b))
