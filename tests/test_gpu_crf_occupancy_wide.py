"""-m gpu: the LDS-resident CRF walks (fcd_set_crf_lattice_wide: crf_forward_walk_lds inside crfp_fwd_kernel<8>,
crfp_occ_walk_lds inside crfp_back_kernel<8, 2, 4>) and the CRF-CTC loss beyond 511 labels on the device.  The table of
tests/crf_occupancy_wide_cases.py on torch device tensors against the float64 restatement; several workspace groups; the
boundary of what one exponent per row holds; crf_ctc_loss on training chunks of 1300 and 1040 rows with half as many
labels, compared as tests/test_gpu_crf_occupancy.py compares its 600-row chunks, on one read of a model-sized state space,
and on a labelling the walk gives up next to one that keeps its value.  On a tree without the feature every test here
fails: `wide` does not exist and the loss raises FCD_E_UNSUPPORTED."""
import math

import numpy as np
import pytest

import crf_lattice_reference as R
import crf_marginals_reference as M
import crf_occupancy_cases as OC
import crf_occupancy_reference as O
import crf_occupancy_wide_cases as WC
import crf_transitions_reference as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("case", WC.CASES, ids=[c["name"] for c in WC.CASES])
def test_cases_on_device_tensors(fcd, case):
    WC.run_case(fcd, WC.build_case(case), device="cuda")


def test_workspace_limit_groups(fcd):
    WC.workspace_limit_groups(fcd, device="cuda")


def test_a_training_chunk_of_an_untrained_network_holds(fcd):
    WC.holds(fcd, device="cuda")


def test_six_rows_per_label_are_given_up(fcd):
    WC.given_up(fcd, device="cuda")


def test_the_switch_is_off_after_the_call(fcd):
    """wide=True does not outlive its call, an error included: 513 states are refused through _dev, nothing is written"""
    import torch
    from fast_ctc_decode_amd import _native as nat
    dev = torch.device("cuda")
    args = (torch.full((1, 513, 4, 5), 0.2, device=dev), torch.ones((1, 4), device=dev),
            torch.ones((1, 513), dtype=torch.uint8, device=dev), [300])
    assert math.isfinite(float(fcd.crf_score_batch_raw(*args, wide=True)[0, 0]))
    with pytest.raises(nat.NativeError) as e:
        fcd.crf_score_batch_raw(torch.zeros((1, 513, 4, 10), device=dev), *args[1:], wide=True)
    assert e.value.code == nat.E_UNSUPPORTED and "crf_score_wide: more than 8 labels" in str(e.value)
    out = torch.full((1, 1, 513, 4, 5), 77.0, device=dev)
    with pytest.raises(nat.NativeError) as e:
        fcd.crf_occupancy_batch_raw(*args, out=out)
    assert e.value.code == nat.E_UNSUPPORTED and "exceeds 512 states: use a band" in str(e.value)
    assert bool((out == 77.0).all())


# ---- crf_ctc_loss -------------------------------------------------------------------------------------------------------
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


def _compare(fcd, x, labels, lens, lengths):
    """loss within 2^-20 max(1, |loss|) of the float64 recurrences; gradient against occupancy64 - marginals64 within the
    occupancies' tolerance at occ = 1, the mass a row may have lost at the call's J states per lane, the rounding of the
    posteriors to occupancy64's float32 interface and the marginals' allowance; zero on rows t >= T_r; no read given up"""
    import torch
    B, T, S, N = x.shape
    J = -(-(min(T, labels.shape[1]) + 1) // 64)
    assert J >= 9, "the call must walk the LDS-resident window"
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    loss = fcd.crf_ctc_loss(xd, torch.from_numpy(labels).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(lengths).cuda())
    loss.sum().backward()
    l, g = loss.detach().cpu().numpy(), xd.grad.cpu().numpy().astype(np.float64)
    for b in range(B):
        Tr, L = int(lengths[b]), int(lens[b])
        xb = x[b, :Tr].astype(np.float64)
        tr = TR.transitions64(xb)
        s0 = R.trajectory(tr["init"].astype(np.float32), [], S, N)[0]
        want = M.logz64(xb) - _numerator64(xb, s0, labels[b, :L])
        ref = O.occupancy64(tr["probs"].astype(np.float32), tr["init"].astype(np.float32), labels[b, :L])
        grad = M.marginals64(xb)["marg"] - ref["occ"]
        allow = OC.tolerance(Tr, L + 1, 1.0) + OC.lost(Tr, J) + (Tr + 1) * 2.0 ** -24 + 2.0 ** -18
        assert math.isfinite(l[b]), (b, "the read was given up")
        worst = float(np.abs(g[b, :Tr] - grad).max())
        print("crf_ctc_loss S=%d chunk %d rows, %d labels: loss %.6f (float64 %.6f), largest gradient difference %.3g, allowance %.3g"
              % (S, Tr, L, l[b], want, worst, allow))
        assert abs(l[b] - want) <= 2.0 ** -20 * max(1.0, abs(want))
        assert worst <= allow and (g[b, Tr:] == 0).all()


def test_crf_ctc_loss_on_training_chunks_beyond_511_labels(fcd):
    """1300 rows and 650 labels, 1040 rows and 520: scores N(0, 1) that support no labelling, S = 4, N = 5"""
    rng = np.random.default_rng(1300)
    x = rng.standard_normal((2, 1300, 4, 5)).astype(np.float32)
    lengths, lens = np.array([1300, 1040], np.int64), np.array([650, 520], np.int32)
    labels = rng.integers(1, 5, (2, 650)).astype(np.uint8)
    _compare(fcd, x, labels, lens, lengths)


def test_crf_ctc_loss_at_a_model_sized_state_space(fcd):
    """S = 1024, N = 5: 600 rows, 520 labels, one read -- the S * N row of 20 KiB next to the window's rows"""
    rng = np.random.default_rng(1024)
    x = rng.standard_normal((1, 600, 1024, 5)).astype(np.float32)
    labels = rng.integers(1, 5, (1, 520)).astype(np.uint8)
    _compare(fcd, x, labels, np.array([520], np.int32), np.array([600], np.int64))


def test_crf_ctc_loss_gives_up_a_wide_lattice_the_rows_cannot_hold(fcd):
    """Uniform scores against 520 labels in 3000 rows are beyond what rows with one float32 exponent hold: the loss and the
    gradient of that read are NaN.  The 700-row read next to it keeps its value, known in closed form: logZ = ln(S N^T), and
    the labelling's C(700, 520) alignments each score 0."""
    import torch
    rng = np.random.default_rng(78)
    T = 3000
    x = torch.zeros((2, T, 4, 5), device="cuda", requires_grad=True)
    labels = torch.from_numpy(rng.integers(1, 5, (2, 520)).astype(np.uint8)).cuda()
    lens = torch.tensor([520, 520], dtype=torch.int32, device="cuda")
    lengths = torch.tensor([T, 700], dtype=torch.int64, device="cuda")
    loss = fcd.crf_ctc_loss(x, labels, lens, lengths)
    loss.sum().backward()
    l, g = loss.detach().cpu().numpy(), x.grad.cpu().numpy().astype(np.float64)
    assert math.isnan(l[0]) and np.isnan(g[0]).all()
    want = math.log(4.0) + 700 * math.log(5.0) - (math.lgamma(701) - math.lgamma(521) - math.lgamma(181))
    assert abs(l[1] - want) <= 2.0 ** -20 * want
    assert np.abs(g[1, :700].sum(axis=(1, 2))).max() <= OC.lost(700, 9) + 2.0 ** -18 and (g[1, 700:] == 0).all()
