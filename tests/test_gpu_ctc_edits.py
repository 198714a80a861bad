"""-m gpu: the edit-likelihood kernels (csrc/ctc_posterior.hip: edit_back_kernel) on the device.  The cases of
tests/ctc_edits_cases.py on torch device tensors (fcd_ctc_edits_dev) and on numpy (fcd_ctc_edits_host) against the
restatement (tests/ctc_edits_reference.py); the edge rows through _dev into poisoned outputs; consistency with ctc_score of
the edited labellings; EditResult.best; the limits; and the search -> edits pipeline under set_overlap(4) with no join in
between."""
import ctypes as C
import math

import numpy as np
import pytest

import ctc_edits_cases as EC
import ctc_edits_reference as ER
import ctc_posterior_cases as PC
import ctc_score_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.fixture(scope="module")
def cases(fcd):
    return {c[0]: EC.build_case(fcd, c) for c in EC.CASES}  # built once, shared, never changed


@pytest.mark.parametrize("name", [c[0] for c in EC.CASES])
def test_cases_on_device_tensors(fcd, cases, name):
    EC.run_case(fcd, cases[name], device="cuda")


@pytest.mark.parametrize("name", [c[0] for c in EC.CASES])
def test_cases_on_numpy(fcd, cases, name):
    EC.run_case(fcd, cases[name])


def test_edge_rows_into_uninitialised_outputs(fcd):
    """straight through fcd_ctc_edits_dev: outputs from torch.empty, poisoned -- every entry k < len and g <= len is
    written, no other"""
    import torch
    from fast_ctc_decode_amd import _native as nat
    x, labels, lens, lengths = PC.edge_batch()
    dev = torch.device("cuda")
    xd, ld, nd, td = (torch.from_numpy(a).to(dev) for a in (x, labels, lens.view(np.int32), lengths))
    dele = torch.empty((10, 8), dtype=torch.float32, device=dev).fill_(77.0)
    ins = torch.empty((10, 9, 3), dtype=torch.float32, device=dev).fill_(77.0)
    logp = torch.empty(10, dtype=torch.float64, device=dev).fill_(77.0)
    h = nat.default_handle(0)
    h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    b = nat.Batch(xd.data_ptr(), 10, 6, 1, 4, 24, 4, 0, 1, td.data_ptr())
    y = nat.Labellings(ld.data_ptr(), nd.data_ptr(), None, None, 1, 8)
    out = nat.Edits(dele.data_ptr(), ins.data_ptr(), logp.data_ptr())
    assert h.lib.fcd_ctc_edits_dev(h.ptr, C.byref(b), C.byref(y), 1, 0, C.byref(out)) == nat.OK
    torch.cuda.synchronize()
    EC.check_edges(dele.cpu().numpy(), ins.cpu().numpy(), logp.cpu().numpy(), x, labels, lens, lengths, 77.0)


def test_stray_nan_and_inf(fcd):
    """a NaN or an infinity in a cell that only a shortened labelling reads stays out of logp and of every other entry"""
    import torch
    for x, y, bad in EC.stray_cases():
        xd, yd, nd = torch.from_numpy(x[None]).cuda(), torch.from_numpy(y[None]).cuda(), torch.tensor([3], dtype=torch.int32).cuda()
        got = fcd.ctc_edits_batch_raw(xd, yd, nd).cpu()
        score = float(fcd.ctc_score_batch_raw(xd, yd, nd).cpu()[0, 0])
        EC.check_stray(got.deletion[0, 0, :3], got.insertion[0, 0, :4], got.logp[0, 0], score, x, y, bad)


def test_consistent_with_ctc_score(fcd):
    """exact mode, on the device: exp(deletion[k]) P(y) is ctc_score of the shortened labelling, one insertion per
    labelling ctc_score of the lengthened one -- each within the sum of the two tolerances"""
    import torch
    rng = np.random.default_rng(10)
    x = SC.posteriors(rng, 4, 30, 5)
    lengths = np.array([30, 17, 8, 26], np.int64)
    xd = torch.from_numpy(x).cuda()
    r = fcd.beam_search_batch_raw(xd, 5, 0.0, lengths=torch.from_numpy(lengths).cuda())
    got = r.ctc_edits(xd, lengths=torch.from_numpy(lengths).cuda()).cpu()
    r = r.cpu()
    for b in range(4):
        n, Tr = int(r.out_len[b]), int(lengths[b])
        y = r.labels[b, :n].tolist()
        variants = [(y[:k] + y[k + 1:], float(got.deletion[b, 0, k])) for k in range(n)]
        g, c = int(rng.integers(n + 1)), int(rng.integers(1, 5))
        variants.append((y[:g] + [c] + y[g:], float(got.insertion[b, 0, g, c - 1])))
        lab = np.zeros((len(variants), 31), np.uint8)
        for j, (v, _) in enumerate(variants):
            lab[j, :len(v)] = v
        sc = fcd.ctc_score_batch_raw(np.repeat(x[b:b + 1], len(variants), 0), lab, [len(v) for v, _ in variants],
                                     lengths=np.full(len(variants), Tr))
        for j, (v, ratio) in enumerate(variants):
            want = sc[j, 0] - got.logp[b, 0]
            if math.isinf(want):
                assert ratio == want
            elif want >= EC.FLOOR:
                assert abs(ratio - want) <= EC.tolerance(Tr, want) + 2 * SC.tolerance(Tr), (b, j, ratio, want)


def test_best_edit(fcd):
    """EditResult.best of device results against the best labelling of the restatement, substitutions included"""
    import torch

    import ctc_posterior_reference as PR
    rng = np.random.default_rng(11)
    x = SC.posteriors(rng, 6, 24, 5)
    r = fcd.beam_search_batch_raw(x, 5, 0.0)
    labels, lens = r.labels.copy(), r.out_len.copy()
    for b in range(1, 6):  # spoil five of the six labellings by one edit each, so that an edit is worth making
        n = int(lens[b])
        lab, _ = SC.edit(rng, labels[b, :n].tolist(), list(range(n)), 5, 24)
        labels[b] = 0
        labels[b, :len(lab)] = lab
        lens[b] = len(lab)
    xd, ld, nd = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(lens.view(np.int32)).cuda()
    ed = fcd.ctc_edits_batch_raw(xd, ld, nd)
    po = fcd.ctc_posterior_batch_raw(xd, ld, nd)
    plain, full = ed.best(nd), ed.best(nd, po, ld)
    compared = 0
    for b in range(6):
        n = int(lens[b])
        y = labels[b, :n]
        d, ins, lp = ER.ctc_edits(x[b], y)
        post, _ = PR.ctc_posterior(x[b], y)
        with np.errstate(all="ignore"):
            sub = np.log(post) - np.log(post[np.arange(n), y.astype(int) - 1])[:, None]
        # (a substitution's log-ratio is the logarithm of a ratio of two posteriors, each within 16 T 2^-24 of its value)
        for got, sb, extra in ((plain, None, 0.0), (full, sub, 32 * 24 * 2.0 ** -24)):
            want, want_val, decided = EC.best_variant(y, d, ins, 24, sb, extra)
            if not decided:
                continue
            compared += 1
            have = EC.apply_edit(y, int(got[0][b, 0]), int(got[1][b, 0]), int(got[2][b, 0]))
            assert have == want, (b, want, [a[b, 0] for a in got])
            assert abs(got[3][b, 0] - want_val) <= EC.tolerance(24, want_val) + extra
    print("ctc_edits: best edit compared on %d of 12 (labelling, with / without substitutions) pairs" % compared)
    assert compared >= 10


def test_limits(fcd):
    import torch
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(6)
    with pytest.raises(nat.NativeError) as e:  # 511 states
        fcd.ctc_edits_batch_raw(torch.from_numpy(SC.posteriors(rng, 1, 255, 5)).cuda(), torch.ones((1, 255), dtype=torch.uint8).cuda(),
                                torch.tensor([5], dtype=torch.int32).cuda())
    assert e.value.code == nat.E_UNSUPPORTED and "ctc_edits" in str(e.value) and "use a band" in str(e.value)
    with pytest.raises(nat.NativeError) as e:  # N - 1 = 9
        fcd.ctc_edits_batch_raw(torch.from_numpy(SC.posteriors(rng, 1, 20, 10)).cuda(), torch.ones((1, 20), dtype=torch.uint8).cuda(),
                                torch.tensor([5], dtype=torch.int32).cuda())
    assert e.value.code == nat.E_UNSUPPORTED
    h = nat.default_handle(0)
    x = torch.from_numpy(SC.posteriors(rng, 2, 10, 5)).cuda()
    lab, lens = torch.ones((2, 10), dtype=torch.uint8).cuda(), torch.tensor([3, 4], dtype=torch.int32).cuda()
    de, ins = torch.zeros((2, 10)).cuda(), torch.zeros((2, 11, 4)).cuda()
    b = nat.Batch(x.data_ptr(), 2, 10, 1, 5, 50, 5, 0, 1, None)
    y = nat.Labellings(lab.data_ptr(), lens.data_ptr(), None, None, 1, 10)
    for out in (None, C.byref(nat.Edits(None, ins.data_ptr(), None)), C.byref(nat.Edits(de.data_ptr(), None, None))):
        assert h.lib.fcd_ctc_edits_dev(h.ptr, C.byref(b), C.byref(y), 1, 0, out) == nat.E_INVALID
    assert h.lib.fcd_ctc_edits_dev(h.ptr, C.byref(b), C.byref(y), 1, 3, C.byref(nat.Edits(de.data_ptr(), ins.data_ptr(), None))) == nat.E_INVALID
    torch.cuda.synchronize()
    assert (de == 0).all() and (ins == 0).all()


def test_search_then_edits_under_overlap(fcd):
    """Four batches back to back: each search goes to an internal stream, each edits call to the handle's stream,
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
            out.append((r, r.ctc_edits(x, band=16), r.ctc_edits(x)))
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
            assert np.array_equal(a0.deletion, a1.deletion, equal_nan=True) and np.array_equal(a0.logp, a1.logp)
            assert np.array_equal(a0.insertion, a1.insertion, equal_nan=True) and np.isfinite(a0.logp).all()
    rc = keep[0][0].cpu()
    x0 = xs[0].cpu().numpy()
    for got, band in zip(overlapped[0], (16, 0)):  # batch 0, two reads, both calls
        for b in (0, 16):
            n = int(rc.out_len[b])
            d, ins, lp = ER.ctc_edits(x0[b], rc.labels[b, :n], True, band, rc.path[b, :n] if band else None)
            assert SC.same(got.logp[b, 0], lp, 120)
            EC.check_one(got.deletion[b, 0, :n], d, 120, ("overlap", band, b, "deletion"))
            EC.check_one(got.insertion[b, 0, :n + 1], ins, 120, ("overlap", band, b, "insertion"))
    h.close()
