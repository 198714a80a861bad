"""-m gpu: the CTC label-occupancy walk (csrc/ctc_posterior.hip) and ctc_loss on the device.  The table of
tests/ctc_occupancy_cases.py on torch device tensors (fcd_ctc_occupancy_dev into prefilled buffers) against the float64
restatement tests/ctc_occupancy_reference.py; the limits through _dev; several workspace groups; the same bits from two
calls; ctc_loss against torch.nn.functional.ctc_loss in float64 on the CPU; a banded loss against the banded ctc_score; and
the search -> occupancy pipeline under set_overlap(2) with no join in between.

ctc_loss's allowances.  The gradient at the logits is softmax - occupancy: an occupancy's own bound(T_r) * occ + lost(T_r)
(include/fcd.h) plus 2^-23 for the float32 softmax.  The loss is -ln P: P carries 3 T_r + 1 roundings, below bound(T_r), and
every float32 log-probability an alignment reads is within 2^-24 of its float64 value relatively, 2^-23 |loss| over a whole
alignment at most."""
import math

import numpy as np
import pytest

import ctc_occupancy_cases as OC
import ctc_occupancy_reference as O
import ctc_score_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("case", OC.CASES, ids=[c["name"] for c in OC.CASES])
def test_cases_on_device_tensors(fcd, case):
    OC.run_case(fcd, OC.build_case(case), device="cuda")


def test_workspace_limit_groups(fcd):
    OC.workspace_limit_groups(fcd, device="cuda")


def test_unsupported_labellings_hold_or_are_given_up(fcd):
    OC.unsupported_labellings(fcd, device="cuda")


def test_same_bits_twice(fcd):
    """every K, written and accumulated: two calls on the same input leave the same bits"""
    import torch
    for name in ("n5_t65_l62_k2", "n9_t129_l126_k4", "n9_t193_l190_k6", "n5_t257_l254_k8", "n9_t130_band4"):
        c = OC.build_case(next(k for k in OC.CASES if k["name"] == name))
        xin, conv, kw = OC._device_inputs(c, "cuda")
        band = c["band"]
        args = (xin, conv(c["labels"]), conv(c["out_len"]), c["collapse"], conv(c["lengths"]), conv(c["paths"]) if band else None, band)
        a, b = fcd.ctc_occupancy_batch_raw(*args), fcd.ctc_occupancy_batch_raw(*args)
        assert torch.equal(a.occupancy.view(torch.int32), b.occupancy.view(torch.int32)), name
        assert torch.equal(a.logp.view(torch.int64), b.logp.view(torch.int64))
        base = torch.full_like(a.occupancy, 0.125)
        u = fcd.ctc_occupancy_batch_raw(*args, out=base.clone(), scale=-1.0, accumulate=True)
        v = fcd.ctc_occupancy_batch_raw(*args, out=base.clone(), scale=-1.0, accumulate=True)
        assert torch.equal(u.occupancy.view(torch.int32), v.occupancy.view(torch.int32)), name


def test_limits_through_dev(fcd):
    """a window of 511 states and 9 labels: unsupported, the message says why, nothing is written"""
    import torch
    from fast_ctc_decode_amd import _native as nat
    f = fcd.ctc_occupancy_batch_raw
    dev = torch.device("cuda")
    out = torch.full((1, 1, 255, 5), 77.0, device=dev)
    with pytest.raises(nat.NativeError) as e:
        f(torch.zeros((1, 255, 5), device=dev), torch.ones((1, 255), dtype=torch.uint8, device=dev), [5], out=out)
    assert e.value.code == nat.E_UNSUPPORTED and "ctc_occupancy" in str(e.value) and "use a band" in str(e.value)
    with pytest.raises(nat.NativeError) as e:
        f(torch.zeros((1, 8, 10), device=dev), torch.ones((1, 8), dtype=torch.uint8, device=dev), [5])
    assert e.value.code == nat.E_UNSUPPORTED and "more than 8 labels" in str(e.value)
    assert bool((out == 77.0).all())
    with pytest.raises(TypeError):
        f(torch.zeros((1, 8, 5), device=dev), torch.ones((1, 8), dtype=torch.uint8, device=dev), [5], out=np.zeros((1, 8, 5), np.float32))


# ---- ctc_loss -----------------------------------------------------------------------------------------------------------
_loss_cases = {}


def _loss_case(B, T, N, L):
    """logits, labellings and the float64 CPU reference of a case, computed once: torch.nn.functional.ctc_loss through
    log_softmax, its gradient at the logits, and the restatement's occupancies (for the allowance)"""
    import torch
    key = (B, T, N, L)
    if key in _loss_cases:
        return _loss_cases[key]
    rng = np.random.default_rng(100 * T + N)
    logits = (rng.standard_normal((B, T, N)) * 2.0).astype(np.float32)
    lengths = np.array([T, T - 3, max(T // 2, 1)][:B], np.int64)
    lens = np.array([min(L, int(l) // 2) for l in lengths], np.int64)
    labels = np.zeros((B, L), np.uint8)
    for b in range(B):
        labels[b, :lens[b]] = rng.integers(1, N, lens[b])
    x = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    lp = torch.log_softmax(x, -1)
    loss = torch.nn.functional.ctc_loss(lp.permute(1, 0, 2), torch.from_numpy(labels.astype(np.int64)), torch.from_numpy(lengths),
                                        torch.from_numpy(lens), blank=0, reduction="none")
    loss.sum().backward()
    p = torch.softmax(x.detach(), -1).numpy()
    occ = np.zeros((B, T, N))
    for b in range(B):
        Tr = int(lengths[b])
        occ[b, :Tr] = O.occupancy64(p[b, :Tr], labels[b, :lens[b]])["occ"]
    _loss_cases[key] = dict(logits=logits, lengths=lengths, lens=lens, labels=labels, loss=loss.detach().numpy(),
                            grad=x.grad.numpy(), occ=occ)
    return _loss_cases[key]


@pytest.mark.parametrize("time_major", [False, True], ids=["read_major", "time_major"])
@pytest.mark.parametrize("B,T,N,L", [(3, 40, 5, 20), (2, 130, 9, 60)])
def test_ctc_loss_against_torch(fcd, B, T, N, L, time_major):
    import torch
    c = _loss_case(B, T, N, L)
    K = OC.states_per_lane(T, L, 0)
    xd = torch.from_numpy(c["logits"]).cuda()
    if time_major:  # a (T, B, N) network output, seen read by read
        xd = xd.permute(1, 0, 2).contiguous()
    xd.requires_grad_(True)
    lp = torch.log_softmax(xd, -1)
    loss = fcd.ctc_loss(lp.permute(1, 0, 2) if time_major else lp, torch.from_numpy(c["labels"]).cuda(),
                        torch.from_numpy(c["lens"].astype(np.int32)).cuda(), torch.from_numpy(c["lengths"]).cuda())
    assert loss.dtype == torch.float64 and tuple(loss.shape) == (B,)
    loss.sum().backward()
    got_loss = loss.detach().cpu().numpy()
    got = (xd.grad.permute(1, 0, 2) if time_major else xd.grad).cpu().numpy().astype(np.float64)
    for b in range(B):
        Tr = int(c["lengths"][b])
        allow_loss = OC.bound(Tr, K) + 2.0 ** -23 * abs(c["loss"][b])
        allow = OC.tolerance(Tr, K, c["occ"][b, :Tr]) + 2.0 ** -23
        diff = np.abs(got[b, :Tr] - c["grad"][b, :Tr])
        print("ctc_loss B=%d T=%d N=%d read %d: loss %.6f (torch float64 %.6f, allowance %.3g), largest gradient difference %.3g "
              "(allowance %.3g and up)" % (B, T, N, b, got_loss[b], c["loss"][b], allow_loss, diff.max(), allow.min()))
        assert abs(got_loss[b] - c["loss"][b]) <= allow_loss
        assert (diff <= allow).all()
        assert (got[b, Tr:] == 0).all()  # the gradient is zero on rows t >= T_r


def test_ctc_loss_banded_is_the_banded_score_and_its_gradient(fcd):
    """band = 4 around the decoded path: the loss is ctc_score's banded value bit for bit (the same float32 posteriors), and
    the gradient by the log-probabilities is minus the banded occupancies of the restatement"""
    import torch
    rng = np.random.default_rng(21)
    x = SC.posteriors(rng, 3, 130, 5)
    lengths = np.array([130, 127, 64], np.int64)
    lp = torch.from_numpy(x).cuda().log().requires_grad_(True)
    p = lp.detach().exp()
    r = fcd.beam_search_batch_raw(p, 5, 0.0, lengths=torch.from_numpy(lengths).cuda())
    for collapse in (True, False):
        lp.grad = None
        loss = fcd.ctc_loss(lp, r.labels, r.out_len, torch.from_numpy(lengths).cuda(), collapse, r.path, 4)
        score = fcd.ctc_score_batch_raw(p, r.labels, r.out_len, collapse, torch.from_numpy(lengths).cuda(), r.path, 4)
        assert torch.equal((-loss.detach()).view(torch.int64), score[:, 0].view(torch.int64))
        loss.backward(torch.tensor([1.0, 0.5, 2.0], dtype=torch.float64, device="cuda"))
        g = lp.grad.cpu().numpy().astype(np.float64) / np.array([1.0, 0.5, 2.0])[:, None, None]
        rc, p32 = r.cpu(), p.cpu().numpy()
        for b in range(3):
            n, Tr = int(rc.out_len[b]), int(lengths[b])
            ref = O.occupancy64(p32[b, :Tr], rc.labels[b, :n], collapse, 4, rc.path[b, :n])
            assert math.isfinite(ref["logp"]) and SC.same(-float(loss.detach()[b]), ref["logp"], Tr)
            assert (np.abs(-g[b, :Tr] - ref["occ"]) <= OC.tolerance(Tr, 2, ref["occ"])).all(), (collapse, b)
            assert (g[b, Tr:] == 0).all()


def test_ctc_loss_rows_without_a_value(fcd):
    """more labels than rows: loss +inf and a zero gradient; a labelling its read does not support (uniform posteriors, 50
    labels in 1000 rows): given up, loss NaN and a NaN gradient; the supported read between them keeps its value; float16
    log-probabilities get a float16 gradient"""
    import torch
    rng = np.random.default_rng(33)
    T, L = OC.GIVEN_UP
    x = rng.random((3, T, 5))
    x = (x / x.sum(-1, keepdims=True)).astype(np.float32)
    labels = rng.integers(1, 5, (3, L)).astype(np.uint8)
    lens, lengths = np.array([L, 20, 30], np.int32), np.array([T, 90, 29], np.int64)
    lp = torch.from_numpy(x).cuda().log().requires_grad_(True)
    loss = fcd.ctc_loss(lp, torch.from_numpy(labels).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(lengths).cuda())
    loss.sum().backward()
    l, g = loss.detach().cpu().numpy(), lp.grad.cpu().numpy().astype(np.float64)
    assert math.isnan(l[0]) and np.isnan(g[0]).all()
    ref = O.occupancy64(lp.detach().exp().cpu().numpy()[1, :90], labels[1, :20])
    assert SC.same(-l[1], ref["logp"], 90) and (np.abs(-g[1, :90] - ref["occ"]) <= OC.tolerance(90, 2, ref["occ"])).all()
    assert (g[1, 90:] == 0).all()
    assert l[2] == math.inf and (g[2] == 0).all()
    half = lp.detach()[1:2, :90].half().requires_grad_(True)
    fcd.ctc_loss(half, torch.from_numpy(labels[1:2]).cuda(), torch.from_numpy(lens[1:2]).cuda()).sum().backward()
    assert half.grad.dtype == torch.float16 and bool(torch.isfinite(half.grad).all())
    with pytest.raises(TypeError):
        fcd.ctc_loss(x, labels, lens)  # numpy: the loss is a torch function


def test_search_then_ctc_occupancy_under_overlap(fcd):
    """Four batches back to back under set_overlap(2): each search goes to an internal stream, each occupancy call to the
    handle's stream, ordered by the library behind the searches in flight; the same bits as in order."""
    import torch
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(12)
    xs = [torch.from_numpy(SC.posteriors(rng, 32, 120, 5)).cuda() for _ in range(4)]
    h = nat.default_handle(0)

    def pipeline():
        out = []
        for x in xs:
            r = fcd.beam_search_batch_raw(x, 8, 0.0)
            out.append((r, r.ctc_occupancy(x, band=16), r.ctc_occupancy(x)))
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        h.overlap_join()
        torch.cuda.synchronize()
        return [(a.cpu(), b.cpu()) for _, a, b in out], out

    in_order, _ = pipeline()
    h.set_overlap(2)
    try:
        overlapped, keep = pipeline()
    finally:
        h.set_overlap(0)
    for pair0, pair1 in zip(in_order, overlapped):
        for a0, a1 in zip(pair0, pair1):
            assert np.array_equal(a0.logp, a1.logp) and np.isfinite(a0.logp).all()
            assert np.array_equal(a0.occupancy.view(np.uint32), a1.occupancy.view(np.uint32))
    rc = keep[0][0].cpu()
    x0 = xs[0].cpu().numpy()
    for got, band in zip(overlapped[0], (16, 0)):  # batch 0, two reads, both calls
        K = OC.states_per_lane(120, rc.labels.shape[-1], band)
        for b in (0, 17):
            n = int(rc.out_len[b])
            ref = O.occupancy64(x0[b], rc.labels[b, :n], True, band, rc.path[b, :n] if band else None)
            assert math.isfinite(ref["logp"]) and SC.same(got.logp[b, 0], ref["logp"], 120)
            assert (np.abs(got.occupancy[b, 0] - ref["occ"]) <= OC.tolerance(120, K, ref["occ"])).all(), (band, b)
