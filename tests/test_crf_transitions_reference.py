"""CPU-only: the restatements of the CRF transition probabilities (tests/crf_transitions_reference.py, the specification of
fcd_crf_transition_probs_* in include/fcd.h) against the enumeration of every start state and symbol sequence of tiny cases:
the path identity init[s0] prod_t p[t][s_t][a_t] = exp(sum_t x[t][s_t][a_t] - logZ), the two score layouts as mutually
inverse permutations, the best path under the scores being the best path under the outputs, and the float32 arithmetic's
distance to the float64 formulas on the table the kernel is checked on."""
import numpy as np
import pytest

import crf_transitions_cases as TC
import crf_transitions_reference as R


def tiny_cases():
    rng = np.random.default_rng(5)
    out = []
    for S, N in ((2, 2), (4, 2), (2, 3), (4, 3), (6, 3), (8, 3), (4, 5), (8, 5)):
        for T in (1, 3, 5):
            if N ** T * S > 30000:
                T = 3
            for flavour in ("plain", "neg_inf", "dead"):
                x = R.random_scores(rng, T, S, N, sd=2.0, n_neg_inf=0 if flavour == "plain" else max(1, S * N * T // 8),
                                    dead=(T - 1, S - 1) if flavour == "dead" else None)
                out.append(("S%d_N%d_T%d_%s" % (S, N, T, flavour), x))
    return out


TINY = tiny_cases()


@pytest.mark.parametrize("name,x", TINY, ids=[c[0] for c in TINY])
def test_path_identity_by_enumeration(name, x):
    ref = R.transitions64(x)
    assert ref["ok"]
    paths = R.enumerate_paths(x)
    total, worst = 0.0, 0.0
    best_score, best_prob = (-np.inf, None), (-np.inf, None)
    with np.errstate(divide="ignore"):
        for s0, sym, states, score in paths:
            prob = ref["init"][s0]
            for t, a in enumerate(sym):
                prob *= ref["probs"][t, states[t], a]
            total += prob
            if score == -np.inf:
                assert prob == 0.0
                continue
            worst = max(worst, abs(np.log(prob) - (score - ref["logz"])))
            if score > best_score[0]:
                best_score = (score, (s0, sym))
            if prob > best_prob[0]:
                best_prob = (prob, (s0, sym))
    assert abs(total - 1.0) < 1e-12 and worst < 1e-12, (total, worst)
    # the path with the largest score sum is the path with the largest init * prod p
    assert best_score[1] == best_prob[1]
    # logZ is ln of the sum over all paths of exp(score)
    scores = np.array([p[3] for p in paths])
    m = scores.max()
    assert abs(m + np.log(np.exp(scores - m).sum()) - ref["logz"]) < 1e-12


@pytest.mark.parametrize("S,N", [(2, 2), (3, 2), (4, 3), (6, 3), (8, 5), (12, 5), (8, 9), (64, 5)])
def test_layouts_are_mutually_inverse_permutations(S, N):
    rng = np.random.default_rng(S * 16 + N)
    x = rng.standard_normal((3, S, N))
    xd = R.source_to_dest(x)
    assert np.array_equal(R.dest_to_source(xd), x) and np.array_equal(R.source_to_dest(R.dest_to_source(x)), x)
    for t in range(3):
        assert np.array_equal(np.sort(xd[t].ravel()), np.sort(x[t].ravel()))
    # the header's formula, element by element
    nb = N - 1
    for s in range(S):
        assert xd[0, s, 0] == x[0, s, 0]
        for j in range(nb):
            assert x[0, s, j + 1] == xd[0, (s * nb) % S + j, 1 + (s * nb) // S]
    # ... and the other way: entry 1 + i of state s' comes from s' div nb + i (S / nb)
    for s2 in range(S):
        for i in range(nb):
            assert xd[0, s2, 1 + i] == x[0, s2 // nb + i * (S // nb), 1 + s2 % nb]


def test_dead_states_and_failures():
    rng = np.random.default_rng(9)
    x = R.random_scores(rng, 4, 4, 3, dead=(0, 2))
    for fn in (R.transitions64, R.transitions32):
        r = fn(x)
        assert r["ok"] and r["init"][2] == 0.0 and (r["probs"][0, 2] == 0.0).all()
        assert abs(r["init"].sum() - 1.0) < 1e-6
    x[2] = -np.inf  # a row nothing passes
    assert not R.transitions64(x)["ok"] and not R.transitions32(x)["ok"]
    for v in (np.nan, np.inf):
        y = R.random_scores(rng, 4, 4, 3)
        y[1, 2, 1] = v
        assert not R.transitions64(y)["ok"] and not R.transitions32(y)["ok"]
    e = R.transitions32(np.zeros((0, 6, 3), np.float32))
    assert e["ok"] and np.array_equal(e["init"], np.full(6, np.float32(1) / np.float32(6))) and e["logz"] == np.log(6.0)


def test_the_renormalisation_is_what_keeps_the_digits():
    """without the per-row maximum |beta| grows with T and p loses digits: the long cases of the table tell the two apart"""
    rng = np.random.default_rng(2)
    x = R.random_scores(rng, 300, 64, 5, sd=5.0)
    ref = R.transitions64(x)
    with_c = np.abs(R.transitions32(x)["probs"] - ref["probs"]).max()
    without = np.abs(R.transitions32(x, renormalise=False)["probs"] - ref["probs"]).max()
    print("T=300 S=64 sd=5: err32 %.3g with the row maximum, %.3g without" % (with_c, without))
    assert with_c < 1e-5 and without > 8 * with_c


@pytest.mark.parametrize("case", TC.CASES, ids=[c["name"] for c in TC.CASES])
def test_float32_restatement_on_the_table(case):
    """err32 per case (the unit of the kernel's allowance) and the restatement's own logZ error under the kernel's bound"""
    c = TC.build_case(case)
    for b in range(c["B"]):
        ref, r32 = c["refs"][b], c["refs32"][b]
        assert ref["ok"] and r32["ok"]
        assert abs(r32["logz"] - ref["logz"]) <= TC.logz_bound(ref["logz"]), (r32["logz"], ref["logz"])
    print("%s: err32 = %.3g" % (c["name"], c["err32"]))
    assert c["err32"] < (1e-3 if c.get("shift") else 2e-5)
