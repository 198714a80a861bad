"""-m gpu: the CRF edge marginals (csrc/crf_transitions.hip, crf_marginals_kernel)
on the device.  The table of tests/crf_marginals_cases.py on torch device tensors (fcd_crf_marginals_dev and
crf_marginals_batch_raw) against the float64 restatement (tests/crf_marginals_reference.py), the case whose LDS passes 64 KiB,
the edge cases, the argument errors and limits, the nullable outputs, host and device entry points bit for bit, torch tensors
in and out without a synchronise, one call between overlapping beam searches under set_overlap(4), and crf_logz against torch
autograd of the float64 recurrence.  Offsets past 2^31 elements and 2^32 bytes: tests/test_gpu_far_offsets.py,
test_far_walks."""
import numpy as np
import pytest

import crf_marginals_cases as MC
import crf_marginals_reference as M
import crf_transitions_cases as TC
import crf_transitions_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("case", MC.CASES, ids=[c["name"] for c in MC.CASES])
def test_cases_on_device_tensors(fcd, case):
    MC.run_case(fcd, case, device="cuda")
    print("%s: err32 %.3g, device %.3g" % (case["name"], MC.build_case(case)["merr32"], MC.OBSERVED[case["name"]]))


def test_lds_above_64_kib(fcd):
    MC.run_case(fcd, MC.BIG_LDS, device="cuda")
    print("%s: err32 %.3g, device %.3g" % (MC.BIG_LDS["name"], MC.build_case(MC.BIG_LDS)["merr32"], MC.OBSERVED[MC.BIG_LDS["name"]]))


def test_edge_cases(fcd):
    MC.edge_cases(fcd, device="cuda")


def test_argument_errors_and_limits(fcd):
    MC.argument_errors(fcd, device="cuda")


def test_nullable_outputs_and_untouched_elements(fcd):
    MC.nullable_outputs(fcd, device="cuda")


def test_host_and_device_entry_points_are_bitwise_equal(fcd):
    for name in ("s4_n5_t300_tm", "s64_n5_t300_sd5", "s1024_n3_t130_f16_dest", "s12_n5_t7_dest_padded", "s8_n9_t65_bf16"):
        c = MC.build_case(MC.by_name(name))
        host, dev = MC.call_abi(fcd, c), MC.call_abi(fcd, c, device="cuda")
        for b in range(c["B"]):
            MC.check_read(c, b, host[0][b], host[1][b], float(host[2][b]), host[3][b], ("host", name, b))
        for h, d, what in zip(host, dev, ("marg", "emit", "logz", "status")):
            assert np.array_equal(h, d), (name, what)


def test_tensors_in_and_out_without_a_synchronise(fcd):
    """device tensors in, device tensors out, torch reads them on the same stream: nothing waits in between"""
    import torch
    rng = np.random.default_rng(33)
    x = TC.peaked_scores(rng, 4, 90, 64, 5)
    xd = torch.from_numpy(x).cuda().half()
    r = fcd.crf_marginals_batch_raw(xd)
    for a in (r.marginals, r.emit, r.logz, r.status):
        assert a.is_cuda
    assert r.marginals.dtype == torch.float32 and r.marginals.shape == (4, 90, 64, 5) and r.emit.shape == (4, 90, 5)
    rows = r.emit.sum(dim=2)                     # reads emit on the device, behind the call
    best = r.marginals.flatten(2).max(dim=2).values  # the likeliest edge of every row
    rc, rows, best = r.cpu(), rows.cpu().numpy(), best.cpu().numpy()
    assert np.abs(rows - 1.0).max() < 1e-5
    x16 = xd.cpu().float().numpy()
    for b in range(4):
        ref = M.marginals64(x16[b])
        assert int(rc.status[b]) == 0 and abs(rc.logz[b] - ref["logz"]) <= MC.logz_bound(ref["logz"])
        assert np.abs(rc.marginals[b] - ref["marg"]).max() < 1e-5 and np.abs(rc.emit[b] - ref["emit"]).max() < 1e-5
        assert np.abs(best[b] - ref["marg"].reshape(90, -1).max(axis=1)).max() < 1e-5


def test_one_call_between_overlapping_beam_searches(fcd):
    """Four batches back to back under set_overlap(4): the beam searches on internal streams, the marginals of the same
    scores on the handle's stream between them, ordered by the library -- no join in between.  The same results as in order."""
    import torch
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(14)
    xs = [torch.from_numpy(TC.peaked_scores(rng, 32, 120, 4, 5, gap=3.0)).cuda() for _ in range(4)]
    h = nat.default_handle(0)

    def pipeline():
        out = []
        for x in xs:
            tr = fcd.crf_transition_probs_batch_raw(x, out_dtype="float16", time_major_out=True)
            beam = fcd.crf_beam_search_batch_raw(tr.probs, tr.init, 8, 0.0)
            m = fcd.crf_marginals_batch_raw(x, time_major_out=True)
            out.append((m, beam, tr))
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        h.overlap_join()
        torch.cuda.synchronize()
        return [(m.cpu(), b.cpu(), tr.cpu()) for m, b, tr in out], out

    in_order, _ = pipeline()
    h.set_overlap(4)
    try:
        overlapped, keep = pipeline()
    finally:
        h.set_overlap(0)
    for (m0, b0, t0), (m1, b1, t1) in zip(in_order, overlapped):
        assert np.array_equal(m0.marginals, m1.marginals) and np.array_equal(m0.emit, m1.emit)
        assert np.array_equal(m0.logz, m1.logz) and np.array_equal(m0.logz, t0.logz)
        assert (m0.status == 0).all() and (m1.status == 0).all() and (b0.status == 0).all()
        assert np.array_equal(b0.out_len, b1.out_len)
        for b in range(32):  # (entries beyond out_len are not written)
            assert np.array_equal(b0.labels[b, :int(b0.out_len[b])], b1.labels[b, :int(b0.out_len[b])]), b
    x0 = xs[0].cpu().numpy()
    for b in (0, 17):
        ref = M.marginals64(x0[b])
        assert np.abs(in_order[0][0].marginals[b] - ref["marg"]).max() < 1e-5


def _torch_logz64(torch, x, lengths, d):
    """the recurrence of fcd_crf_transition_probs_* in float64 torch operations, read by read -> logz (B,)"""
    out = []
    for b in range(x.shape[0]):
        beta = torch.zeros(x.shape[2], dtype=torch.float64, device=x.device)
        for t in range(int(lengths[b]) - 1, -1, -1):
            beta = torch.logsumexp(x[b, t] + beta[d], dim=1)
        out.append(torch.logsumexp(beta, dim=0))
    return torch.stack(out)


@pytest.mark.parametrize("S,N,T", [(4, 5, 9), (64, 5, 33), (1024, 3, 5)])
def test_crf_logz_against_torch_autograd(fcd, S, N, T):
    import torch
    B = 3
    rng = np.random.default_rng(S + T)
    x = np.stack([R.random_scores(rng, T, S, N) for _ in range(B)])
    lengths = np.array([T, T - 3, T - 1], np.int64)
    d = torch.from_numpy(R.destinations(S, N)).cuda()
    # the allowance of marg on these reads: 4 err32 + 2^-20, as tests/crf_marginals_cases.py computes it
    err32 = 0.0
    for b in range(B):
        ref, r32 = M.marginals64(x[b, :lengths[b]]), M.marginals32(x[b, :lengths[b]])
        err32 = max(err32, float(np.abs(r32["marg"] - ref["marg"]).max()))
    tol = 4 * err32 + 2.0 ** -20

    x64 = torch.from_numpy(x).cuda().double().requires_grad_(True)
    want = _torch_logz64(torch, x64, lengths, d)
    w = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64, device="cuda")
    (want * w).sum().backward()

    xs = torch.from_numpy(x).cuda().requires_grad_(True)
    logz = fcd.crf_logz(xs, torch.from_numpy(lengths).cuda())
    assert logz.dtype == torch.float64 and logz.shape == (B,) and logz.requires_grad
    (logz * w).sum().backward()
    assert xs.grad.dtype == torch.float32 and xs.grad.shape == xs.shape
    g, gw = xs.grad.cpu().numpy().astype(np.float64), x64.grad.cpu().numpy()
    lz, lw = logz.detach().cpu().numpy(), want.detach().cpu().numpy()
    worst = 0.0
    for b in range(B):
        n = int(lengths[b])
        assert abs(lz[b] - lw[b]) <= MC.logz_bound(lw[b]), (b, lz[b], lw[b])
        assert (g[b, n:] == 0).all() and (gw[b, n:] == 0).all(), "the rows beyond a read's length have gradient 0"
        worst = max(worst, float(np.abs(g[b, :n] / float(w[b]) - gw[b, :n] / float(w[b])).max()))
    print("S=%d N=%d T=%d: largest |gradient - autograd| per unit of grad_out %.3g, allowance %.3g" % (S, N, T, worst, tol))
    assert worst <= tol

    # a NaN in one read: that read's gradient is NaN, its rows beyond the length included; the others' bits stay
    y = x.copy()
    y[1, 1, 0, 0] = np.nan
    ys = torch.from_numpy(y).cuda().requires_grad_(True)
    lz2 = fcd.crf_logz(ys, torch.from_numpy(lengths).cuda())
    (lz2 * w).sum().backward()
    g2 = ys.grad.cpu().numpy()
    assert np.isnan(g2[1]).all() and np.isnan(lz2.detach().cpu().numpy()[1])
    assert np.array_equal(g2[0], xs.grad.cpu().numpy()[0]) and np.array_equal(g2[2], xs.grad.cpu().numpy()[2])

    # float16 scores: the gradient comes back in float16; no lengths: every row
    xh = torch.from_numpy(x).cuda().half().requires_grad_(True)
    fcd.crf_logz(xh).sum().backward()
    assert xh.grad.dtype == torch.float16 and xh.grad.shape == xh.shape
    rows = xh.grad.float().sum(dim=(2, 3)).cpu().numpy()
    assert np.abs(rows - 1.0).max() < 4e-3  # (S N float16 roundings of values that sum to 1)
