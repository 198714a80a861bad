"""CPU-only: pins tests/ctc_occupancy_reference.py, the float64 restatement the occupancy walk is held to.  Its rows sum
to 1; its logp is tests/ctc_score_reference.py's; with collapse_repeats its gradient at the logits through log_softmax
(softmax - occ) is the float64 CPU gradient of torch.nn.functional.ctc_loss to 1e-10, and a finite-difference gradient of
the restatement's own logp agrees; at T <= 6 it equals the sum over every alignment, one by one."""
import math

import numpy as np
import pytest

import ctc_occupancy_reference as O
import ctc_score_cases as SC
import ctc_score_reference as R


def _case(seed, T, N, L, homopolymer=False):
    rng = np.random.default_rng(seed)
    x = SC.posteriors(rng, 1, T, N)[0].astype(np.float64)
    y = np.full(L, 1) if homopolymer else rng.integers(1, N, L)
    path = np.sort(rng.choice(T, L, replace=False)) if L <= T else np.arange(L)
    return x, y, path


@pytest.mark.parametrize("collapse", (True, False))
@pytest.mark.parametrize("T,N,L,band", ((1, 3, 0, 0), (1, 3, 1, 0), (7, 5, 7, 0), (30, 5, 11, 0), (30, 5, 11, 2), (40, 2, 9, 3),
                                       (60, 9, 25, 0), (60, 9, 25, 4)))
def test_rows_sum_to_one_and_logp_is_the_score(T, N, L, band, collapse):
    x, y, path = _case(T * 31 + L, T, N, L)
    r = O.occupancy64(x, y, collapse, band, path if band else None)
    want = R.ctc_logp(x, y, collapse, band, path if band else None)
    if not math.isfinite(want):
        assert r["occ"] is None and r["logp"] == want
        return
    assert abs(r["logp"] - want) <= 1e-11 * max(1.0, abs(want))
    assert r["occ"].shape == (T, N) and (r["occ"] >= 0).all()
    assert np.abs(r["occ"].sum(1) - 1.0).max() <= 1e-11
    used = set(int(v) for v in y) | {0}
    assert all((r["occ"][:, c] == 0).all() for c in range(N) if c not in used)


def test_one_alignment_is_one_hot():
    x, y, _ = _case(3, 6, 5, 6)
    y = np.array([1, 2, 1, 3, 4, 2])
    r = O.occupancy64(x, y, True)
    want = np.zeros((6, 5))
    want[np.arange(6), y] = 1.0
    assert np.abs(r["occ"] - want).max() <= 1e-14


def test_rows_without_a_value():
    x, y, _ = _case(5, 6, 4, 3)
    assert O.occupancy64(x, [1, 2, 3, 1, 2, 3, 1])["logp"] == -math.inf            # L > T
    assert O.occupancy64(x, [3, 3, 3, 3], True)["logp"] == -math.inf               # repeats need 7 rows
    assert O.occupancy64(x, [3, 3, 3, 3], False)["occ"] is not None
    assert math.isnan(O.occupancy64(x, [1, 4])["logp"]) and math.isnan(O.occupancy64(x, [0])["logp"])
    assert O.occupancy64(x[:0], [])["logp"] == 0.0 and O.occupancy64(x[:0], [1])["logp"] == -math.inf
    bad = x.copy()
    bad[2, 0] = np.nan
    assert math.isnan(O.occupancy64(bad, y)["logp"]) and O.occupancy64(bad, y)["occ"] is None
    off = x.copy()
    off[2, 3] = np.nan  # label 3 is not in the labelling: no alignment reads it
    r = O.occupancy64(off, [1, 2, 1])
    assert math.isfinite(r["logp"]) and np.array_equal(r["occ"], O.occupancy64(x, [1, 2, 1])["occ"])
    zero = x.copy()
    zero[3] = 0.0
    assert O.occupancy64(zero, y)["logp"] == -math.inf


@pytest.mark.parametrize("collapse", (True, False))
@pytest.mark.parametrize("T,N,y", ((1, 3, []), (1, 3, [2]), (4, 3, [1, 2]), (5, 3, [1, 1, 1]), (6, 3, [1, 1, 1]), (6, 3, [2, 1, 1]),
                                   (5, 4, [3]), (6, 2, [1, 1])))
def test_brute_force(T, N, y, collapse):
    x = SC.posteriors(np.random.default_rng(T * 7 + len(y)), 1, T, N)[0].astype(np.float64)
    P, occ = O.brute_force(x, y, collapse)
    r = O.occupancy64(x, y, collapse)
    if P == 0.0:
        assert r["logp"] == -math.inf and r["occ"] is None
        return
    assert abs(r["logp"] - math.log(P)) <= 1e-12
    assert np.abs(r["occ"] - occ).max() <= 1e-13


@pytest.mark.parametrize("T,N,L,homopolymer", ((12, 5, 4, False), (9, 3, 3, True), (40, 5, 17, False), (130, 9, 60, False)))
def test_gradient_is_torch_ctc_loss(T, N, L, homopolymer):
    """d(-ln P)/d logits = softmax - occ, against torch's float64 CPU autograd through log_softmax and ctc_loss"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(T + L)
    logits = torch.tensor(rng.standard_normal((T, 1, N)) * 2.0, dtype=torch.float64, requires_grad=True)
    y = np.full(L, 1) if homopolymer else rng.integers(1, N, L)
    lp = torch.log_softmax(logits, -1)
    loss = torch.nn.functional.ctc_loss(lp, torch.tensor(y[None]), torch.tensor([T]), torch.tensor([L]), blank=0, reduction="none")
    loss.sum().backward()
    p = torch.softmax(logits.detach(), -1)[:, 0].numpy()
    r = O.occupancy64(p, y, True)
    assert abs(-r["logp"] - float(loss.detach()[0])) <= 1e-10 * max(1.0, abs(float(loss.detach()[0])))
    assert np.abs((p - r["occ"]) - logits.grad[:, 0].numpy()).max() <= 1e-10


@pytest.mark.parametrize("collapse,band", ((True, 0), (False, 0), (True, 2)))
def test_finite_differences_of_the_restatement(collapse, band):
    """occ = d ln P / d ln p, entry by entry, by central differences of the restatement's own logp (band included)"""
    x, y, path = _case(11, 9, 4, 4)
    pth = path if band else None
    r = O.occupancy64(x, y, collapse, band, pth)
    h = 1e-6
    for t in range(9):
        for c in range(4):
            up, dn = x.copy(), x.copy()
            up[t, c] *= math.exp(h)
            dn[t, c] *= math.exp(-h)
            d = (O.occupancy64(up, y, collapse, band, pth)["logp"] - O.occupancy64(dn, y, collapse, band, pth)["logp"]) / (2 * h)
            assert abs(d - r["occ"][t, c]) <= 1e-8, (t, c, d, r["occ"][t, c])
