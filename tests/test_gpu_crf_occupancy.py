"""-m gpu: the CRF edge-occupancy walk (csrc/crf_posterior.hip) and the CRF-CTC loss on the device.  The table of
tests/crf_occupancy_cases.py on torch device tensors (fcd_crf_occupancy_dev into prefilled buffers) against the float64
restatement tests/crf_occupancy_reference.py; the limits through _dev; several workspace groups; crf_ctc_loss against torch
autograd of an independent float64 log-space recurrence on the CPU; and the search -> occupancy pipeline under set_overlap(4)
with no join in between.

crf_ctc_loss's gradient allowance follows the rule of the marginals' tests: 4 err32 + 2^-20 per unit of grad_out, err32 being
the case's largest difference between a float32 numpy restatement of the whole chain (crf_transitions_reference.transitions32
-> crf_marginals_reference.propagate32 and crf_occupancy_reference.occupancy32, and for float16 scores the rounding of
grad_out * G to float16 that ends the chain) and the float64 gradient.  The figures measured on an MI355X are in
INTEGRATION.md section 2m."""
import ctypes as C
import math

import numpy as np
import pytest

import crf_lattice_cases as CC
import crf_lattice_reference as R
import crf_marginals_reference as M
import crf_occupancy_cases as OC
import crf_occupancy_reference as O
import crf_transitions_reference as TR

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


def test_limits_through_dev(fcd):
    """a window of 513 states and an S * N row beyond the LDS: unsupported, the message says why, nothing is written"""
    import torch
    from fast_ctc_decode_amd import _native as nat
    f = fcd.crf_occupancy_batch_raw
    dev = torch.device("cuda")
    with pytest.raises(nat.NativeError) as e:
        f(torch.zeros((1, 1, 8192, 5), device=dev), torch.ones((1, 8192), device=dev), torch.ones((1, 1), dtype=torch.uint8, device=dev), [0])
    assert e.value.code == nat.E_UNSUPPORTED and "crf_occupancy" in str(e.value) and "160 KiB" in str(e.value)
    out = torch.full((1, 1, 512, 4, 5), 77.0, device=dev)
    with pytest.raises(nat.NativeError) as e:
        f(torch.zeros((1, 512, 4, 5), device=dev), torch.ones((1, 4), device=dev), torch.ones((1, 512), dtype=torch.uint8, device=dev), [5], out=out)
    assert e.value.code == nat.E_UNSUPPORTED and "use a band" in str(e.value)
    assert bool((out == 77.0).all())
    # the largest state count of the usual alphabet inside the limit runs: S = 4096 at N = 5, 80 KiB of accumulation row
    rng = np.random.default_rng(3)
    x = CC.posteriors(rng, 1, 6, 4096, 5)
    init = rng.random((1, 4096)).astype(np.float32)
    y = np.array([[2, 1, 4, 0, 0, 0]], np.uint8)
    got = f(torch.from_numpy(x).to(dev), torch.from_numpy(init).to(dev), torch.from_numpy(y).to(dev), [3]).cpu()
    ref = O.occupancy64(x[0], init[0], y[0, :3])
    assert (np.abs(got.occupancy[0, 0] - ref["occ"]) <= OC.tolerance(6, 4, ref["occ"])).all()


# ---- crf_ctc_loss -------------------------------------------------------------------------------------------------------
def _loss64(x, y, s0):
    """torch float64 on the CPU: logZ as crf_marginals_reference.logz64 has it, minus the log-space sum over the alignments of
    y from start state s0 of the raw scores -- differentiable"""
    import torch
    T, S, N = x.shape
    nb = N - 1
    d = torch.from_numpy(TR.destinations(S, N).astype(np.int64))
    beta = torch.zeros(S, dtype=torch.float64)
    for t in range(T - 1, -1, -1):
        beta = torch.logsumexp(x[t] + beta[d], dim=1)
    logz = torch.logsumexp(beta, dim=0)
    L = len(y)
    sig = [s0]
    for v in y:
        sig.append((sig[-1] * nb) % S + v - 1)
    a = {0: torch.zeros((), dtype=torch.float64)}
    for t in range(T):
        n = {}
        for k in range(max(0, L - (T - 1 - t)), min(L, t + 1) + 1):  # (the cone: every cell has a parent)
            terms = []
            if k in a and 0 <= sig[k] < S:
                terms.append(a[k] + x[t, sig[k], 0])
            if k - 1 in a and 0 <= sig[k - 1] < S:
                terms.append(a[k - 1] + x[t, sig[k - 1], y[k - 1]])
            if terms:
                n[k] = torch.logsumexp(torch.stack(terms), dim=0)
        a = n
    return logz - a[L]


_loss_cases = {}


def _loss_case(S, N, T, half, with_start):
    """scores, labellings and the two references of a case, computed once: float64 loss and gradient by torch autograd on the
    CPU, and the float32 numpy restatement of the device's chain"""
    import torch
    key = (S, N, T, half, with_start)
    if key in _loss_cases:
        return _loss_cases[key]
    rng = np.random.default_rng(1000 + S + 7 * T + (1 if half else 0) + (2 if with_start else 0))
    B = 3
    x = np.stack([TR.random_scores(rng, T, S, N, sd=1.5) for _ in range(B)])
    if half:
        x = x.astype(np.float16).astype(np.float32)  # (the values the device reads)
    lengths = np.array([T, max(T - 2, 1), max(T // 2, 1)], np.int64)
    lens = np.array([min(int(l), max(1, int(l) * 2 // 3)) for l in lengths], np.uint32)
    labels = np.zeros((B, T), np.uint8)
    for b in range(B):
        labels[b, :lens[b]] = rng.integers(1, N, lens[b])
    start = rng.integers(0, S, B).astype(np.int64) if with_start else None
    w = np.array([1.0, 0.5, 2.0])
    loss = np.zeros(B)
    grad = np.zeros((B, T, S, N))
    g32 = np.zeros((B, T, S, N), np.float32)
    for b in range(B):
        Tr, y = int(lengths[b]), [int(v) for v in labels[b, :lens[b]]]
        tr = TR.transitions32(x[b, :Tr])
        s0 = int(start[b]) if with_start else R.trajectory(tr["init"], [], S, N)[0]
        xt = torch.tensor(x[b, :Tr], dtype=torch.float64, requires_grad=True)
        lb = _loss64(xt, y, s0)
        lb.backward()
        loss[b], grad[b, :Tr] = float(lb.detach()), xt.grad.numpy()
        first = np.zeros(S, np.float32)
        first[s0] = 1.0
        marg32, _ = M.propagate32(tr["probs"], tr["init"])
        occ32 = O.occupancy32(tr["probs"], first if with_start else tr["init"], y)["occ"]
        g32[b, :Tr] = marg32 - occ32
    if half:  # the chain ends in the dtype of the scores: grad_out * G rounded to float16
        g32 = ((w[:, None, None, None].astype(np.float32) * g32).astype(np.float16).astype(np.float64) / w[:, None, None, None])
    err32 = float(np.abs(g32 - grad).max())
    _loss_cases[key] = dict(x=x, lengths=lengths, lens=lens, labels=labels, start=start, w=w, loss=loss, grad=grad, err32=err32)
    return _loss_cases[key]


@pytest.mark.parametrize("with_start", [False, True], ids=["model_start", "start_states"])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("S,N,T", [(4, 5, 9), (64, 5, 33), (1024, 3, 5)])
def test_crf_ctc_loss_against_autograd(fcd, S, N, T, half, with_start):
    import torch
    c = _loss_case(S, N, T, half, with_start)
    dev = torch.device("cuda")
    xd = torch.from_numpy(c["x"]).to(dev)
    xd = (xd.half() if half else xd).requires_grad_(True)
    start = None if c["start"] is None else torch.from_numpy(c["start"]).to(dev)
    loss = fcd.crf_ctc_loss(xd, torch.from_numpy(c["labels"]).to(dev), torch.from_numpy(c["lens"].view(np.int32)).to(dev),
                            torch.from_numpy(c["lengths"]).to(dev), start)
    assert loss.dtype == torch.float64 and tuple(loss.shape) == (3,)
    loss.backward(torch.from_numpy(c["w"]).to(dev))
    got_loss, got = loss.detach().cpu().numpy(), xd.grad.float().cpu().numpy().astype(np.float64)
    assert xd.grad.dtype == xd.dtype
    worst_loss = float((np.abs(got_loss - c["loss"]) / np.maximum(1.0, np.abs(c["loss"]))).max())
    allow = 4.0 * c["err32"] + 2.0 ** -20
    per_unit = np.abs(got / c["w"][:, None, None, None] - c["grad"])
    print("crf_ctc_loss S=%d N=%d T=%d %s %s: |loss - ref| / max(1, |loss|) = %.3g; gradient: largest difference %.3g, err32 %.3g, "
          "allowance %.3g" % (S, N, T, "f16" if half else "f32", "start_states" if with_start else "model start", worst_loss,
                              per_unit.max(), c["err32"], allow))
    assert worst_loss <= 2.0 ** -20
    assert per_unit.max() <= allow
    for b in range(3):  # the gradient is zero on rows t >= T_r
        assert (got[b, int(c["lengths"][b]):] == 0).all()


def test_crf_ctc_loss_failed_reads(fcd):
    """a NaN score: loss NaN and a NaN gradient for that read, the other reads' bits as they were; a labelling longer than its
    read: loss +inf and a NaN gradient"""
    import torch
    c = _loss_case(4, 5, 9, False, False)
    dev = torch.device("cuda")
    lab, lens, lengths = (torch.from_numpy(a).to(dev) for a in (c["labels"], c["lens"].view(np.int32), c["lengths"]))

    def run(x, lens):
        xd = torch.from_numpy(x).to(dev).requires_grad_(True)
        loss = fcd.crf_ctc_loss(xd, lab, lens, lengths)
        loss.backward(torch.ones(3, dtype=torch.float64, device=dev))
        return loss.detach().cpu().numpy(), xd.grad.cpu().numpy()
    clean_loss, clean_grad = run(c["x"], lens)
    bad = c["x"].copy()
    bad[1, 2, 1, 3] = np.nan
    loss, grad = run(bad, lens)
    assert math.isnan(loss[1]) and np.isnan(grad[1]).all()
    for b in (0, 2):
        assert loss[b].tobytes() == clean_loss[b].tobytes() and grad[b].tobytes() == clean_grad[b].tobytes()
    long_lens = lens.clone()
    long_lens[2] = int(c["lengths"][2]) + 1  # (labels[2] holds zeros there: the length is tested first)
    lab2 = lab.clone()
    lab2[2, :] = 1
    xd = torch.from_numpy(c["x"]).to(dev).requires_grad_(True)
    loss = fcd.crf_ctc_loss(xd, lab2, long_lens, lengths)
    loss.backward(torch.ones(3, dtype=torch.float64, device=dev))
    l, g = loss.detach().cpu().numpy(), xd.grad.cpu().numpy()
    assert l[2] == math.inf and np.isnan(g[2]).all()
    for b in (0, 1):
        assert l[b].tobytes() == clean_loss[b].tobytes() and g[b].tobytes() == clean_grad[b].tobytes()
    with pytest.raises(TypeError):
        fcd.crf_ctc_loss(c["x"], c["labels"], c["lens"])  # numpy: the loss is a torch function


def _numerator64(x, s0, y):
    """ln of the sum over the alignments of y from start state s0 of exp(score), float64 log space, a row at a time"""
    T, S, N = x.shape
    L, nb = len(y), N - 1
    sig = [s0]
    for v in y:
        sig.append((sig[-1] * nb) % S + int(v) - 1)
    sig, ys = np.array(sig), np.array(list(y) + [0])
    a = np.full(L + 1, -np.inf)
    a[0] = 0.0
    for t in range(T):
        stay = a + x[t, sig, 0]
        adv = a[:-1] + x[t, sig[:-1], ys[:-1]]
        a = np.logaddexp(stay, np.concatenate([[-np.inf], adv]))
    return float(a[L])


def test_crf_ctc_loss_on_training_chunks_of_an_untrained_network(fcd):
    """600 rows and 300 labels, 450 rows and 225: scores N(0, 1) that support no labelling -- the shape training starts
    from.  The loss against the float64 log-space recurrences within 2^-20 max(1, |loss|); the gradient against
    occupancy64 - marginals64 (p and init of transitions64, p rounded to float32 for occupancy64's interface: up to (T + 1)
    2^-24 of an occupancy) within the occupancies' tolerance at occ = 1 plus the mass a row may have lost (include/fcd.h)
    plus the marginals' allowance, 2^-18 (tests/crf_marginals_cases.py measures 4 err32 + 2^-20 below that at S = 4);
    no read is given up."""
    import torch
    rng = np.random.default_rng(600)
    T, S, N = 600, 4, 5
    x = rng.standard_normal((2, T, S, N)).astype(np.float32)
    lengths, lens = np.array([600, 450], np.int64), np.array([300, 225], np.int32)
    labels = rng.integers(1, N, (2, 300)).astype(np.uint8)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    loss = fcd.crf_ctc_loss(xd, torch.from_numpy(labels).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(lengths).cuda())
    loss.sum().backward()
    l, g = loss.detach().cpu().numpy(), xd.grad.cpu().numpy().astype(np.float64)
    for b in range(2):
        Tr, L = int(lengths[b]), int(lens[b])
        xb = x[b, :Tr].astype(np.float64)
        tr = TR.transitions64(xb)
        s0 = R.trajectory(tr["init"].astype(np.float32), [], S, N)[0]
        want = M.logz64(xb) - _numerator64(xb, s0, labels[b, :L])
        ref = O.occupancy64(tr["probs"].astype(np.float32), tr["init"].astype(np.float32), labels[b, :L])
        grad = M.marginals64(xb)["marg"] - ref["occ"]
        allow = OC.tolerance(Tr, L + 1, 1.0) + OC.lost(Tr, 8) + (Tr + 1) * 2.0 ** -24 + 2.0 ** -18
        worst = float(np.abs(g[b, :Tr] - grad).max())
        print("crf_ctc_loss chunk %d rows, %d labels: loss %.6f (float64 %.6f), largest gradient difference %.3g, allowance %.3g"
              % (Tr, L, l[b], want, worst, allow))
        assert abs(l[b] - want) <= 2.0 ** -20 * max(1.0, abs(want))
        assert worst <= allow and (g[b, Tr:] == 0).all()


def test_crf_ctc_loss_gives_up_a_lattice_the_rows_cannot_hold(fcd):
    """Uniform scores against 127 labels in 1500 rows are beyond what rows with one float32 exponent hold (include/fcd.h):
    the occupancy walk gives the labelling up, and the loss and the gradient of that read are NaN, not wrong.  The 200-row
    read next to it keeps its value, known in closed form: logZ = ln(S N^T), and the labelling's C(200, 127) alignments
    each score 0."""
    import torch
    rng = np.random.default_rng(77)
    T = 1500
    x = torch.zeros((2, T, 4, 5), device="cuda", requires_grad=True)
    labels = torch.from_numpy(rng.integers(1, 5, (2, 127)).astype(np.uint8)).cuda()
    lens = torch.tensor([127, 127], dtype=torch.int32, device="cuda")
    lengths = torch.tensor([T, 200], dtype=torch.int64, device="cuda")
    loss = fcd.crf_ctc_loss(x, labels, lens, lengths)
    loss.sum().backward()
    l, g = loss.detach().cpu().numpy(), x.grad.cpu().numpy().astype(np.float64)
    assert math.isnan(l[0]) and np.isnan(g[0]).all()
    want = math.log(4.0) + 200 * math.log(5.0) - (math.lgamma(201) - math.lgamma(128) - math.lgamma(74))
    assert abs(l[1] - want) <= 2.0 ** -20 * want
    assert np.abs(g[1, :200].sum(axis=(1, 2))).max() <= OC.lost(200, 2) + 2.0 ** -18 and (g[1, 200:] == 0).all()


def test_search_then_crf_occupancy_under_overlap(fcd):
    """Four batches back to back: each search goes to an internal stream, each occupancy call to the handle's stream,
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
            out.append((r, r.crf_occupancy(x, init, band=16), r.crf_occupancy(x, init)))
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
            assert np.array_equal(a0.logp, a1.logp) and np.isfinite(a0.logp).all()
            # (the same terms; an entry several states share may add them in another order)
            assert np.allclose(a0.occupancy, a1.occupancy, rtol=2.0 ** -20, atol=2.0 ** -100)
    rc = keep[0][0].cpu()
    x0, i0 = xs[0].cpu().numpy(), init.cpu().numpy()
    for got, band in zip(overlapped[0], (16, 0)):  # batch 0, two reads, both calls
        for b in (0, 17):
            n = int(rc.out_len[b])
            ref = O.occupancy64(x0[b], i0[b], rc.labels[b, :n], band, rc.path[b, :n] if band else None)
            assert math.isfinite(ref["logp"]) and abs(got.logp[b, 0] - ref["logp"]) <= CC.tolerance(120)
            W = min(n + 1, 2 * band + 1) if band else n + 1
            assert (np.abs(got.occupancy[b, 0] - ref["occ"]) <= OC.tolerance(120, W, ref["occ"])).all(), (band, b)
