"""CPU-only: tests/nbest_reference.py -- the whole-final-beam restatement the n-best tests compare the kernels with -- is
pinned to the oracle: its hypothesis 0 and its status equal oracle.beam_search_raw / oracle.crf_beam_search on random,
peaky, tied and special-valued (NaN, 0, > 1) inputs, under both tie orders."""
import numpy as np
import pytest

import nbest_reference as NR
from oracle import oracle

ORDERS = ("pdqsort", "stable")
ORACLE_STATUS = {0: NR.OK, 1: NR.RAN_OUT_OF_BEAM, 2: NR.INCOMPARABLE, 100: NR.BAD_STATE}


def plain_cases(seed, n):
    """(x, beam, thr, collapse): random, peaky, quantised (ties) and special-valued posteriors"""
    rng = np.random.default_rng(seed)
    for i in range(n):
        kind = i % 4
        T = int(rng.integers(0, 40))
        N = int(rng.choice([2, 3, 5, 8]))
        if kind == 0:
            x = rng.random((T, N), dtype=np.float32)
            x /= np.maximum(x.sum(-1, keepdims=True), 1e-6)
        elif kind == 1:
            z = rng.normal(size=(T, N)).astype(np.float32) * 4.0
            e = np.exp(z - z.max(-1, keepdims=True))
            x = (e / e.sum(-1, keepdims=True)).astype(np.float32)
        elif kind == 2:
            x = (rng.integers(0, 4, size=(T, N)) / 4.0).astype(np.float32)
        else:
            x = rng.random((T, N), dtype=np.float32)
            if T:
                x[rng.integers(0, T)] = 0.0
                x[rng.integers(0, T), rng.integers(0, N)] = 1.5
                if rng.random() < 0.5:
                    x[rng.integers(0, T), rng.integers(0, N)] = np.nan
        beam = int(rng.choice([1, 2, 5, 8, 12, 32]))
        thr = float(rng.choice([0.0, 0.0, 0.05, 0.3]))
        yield x.astype(np.float32), beam, thr, bool(rng.random() < 0.8)


@pytest.mark.parametrize("order", ORDERS)
def test_plain_hypothesis_0_is_the_oracle(order):
    seen = {NR.OK: 0, NR.RAN_OUT_OF_BEAM: 0, NR.INCOMPARABLE: 0}
    with oracle.unstable_sort(order):
        for x, beam, thr, collapse in plain_cases(11, 240):
            st, hyps = NR.beam_search(x, beam, thr, collapse, stable=order == "stable")
            ost, labels, path, _ = oracle.beam_search_raw(x, beam, thr, collapse)
            assert st == ORACLE_STATUS[ost], (st, ost)
            seen[st] += 1
            if st == NR.OK:
                assert 1 <= len(hyps) <= beam
                assert hyps[0][0] == labels.tolist() and hyps[0][1] == path.tolist()
                assert len({tuple(h[0]) for h in hyps}) == len(hyps)  # distinct labellings
                assert all(h[2] <= 1.0 + 1e-6 or h[2] != h[2] or x.max() > 1 for h in hyps)
            else:
                assert hyps == []
    assert min(seen.values()) > 0, seen


def test_the_tie_orders_differ_on_wide_tied_steps():
    """above 20 candidates the quicksort's order of equal probabilities is not the stable one: the helper must follow"""
    rng = np.random.default_rng(5)
    differ = 0
    for _ in range(12):
        x = (rng.integers(1, 4, size=(60, 5)) / 4.0).astype(np.float32)
        a = NR.beam_search(x, 12, 0.0)
        b = NR.beam_search(x, 12, 0.0, stable=True)
        with oracle.unstable_sort("pdqsort"):
            assert a[1][0][0] == oracle.beam_search_raw(x, 12, 0.0)[1].tolist()
        with oracle.unstable_sort("stable"):
            assert b[1][0][0] == oracle.beam_search_raw(x, 12, 0.0)[1].tolist()
        differ += a != b
    assert differ > 0


def crf_cases(seed, n):
    rng = np.random.default_rng(seed)
    for i in range(n):
        S, N = [(4, 5), (3, 4), (16, 5), (4, 3)][i % 4]
        T = int(rng.integers(1, 30))
        if i % 3 == 2:
            x = (rng.integers(0, 4, size=(T, S, N)) / 4.0).astype(np.float32)
        else:
            x = rng.random((T, S, N), dtype=np.float32)
        init = rng.random(S + (i % 5 == 4), dtype=np.float32)  # one init longer than S: a start state out of range
        if i % 11 == 10:
            init[0] = np.nan
        if i % 13 == 12:
            x[rng.integers(0, T)] = np.nan
        beam = int(rng.choice([1, 3, 5, 16]))
        thr = float(rng.choice([0.0, 0.1]))
        yield x, init, beam, thr


@pytest.mark.parametrize("order", ORDERS)
def test_crf_hypothesis_0_is_the_oracle(order):
    alphabet = "NACGT"
    seen = set()
    with oracle.unstable_sort(order):
        for x, init, beam, thr in crf_cases(23, 160):
            N = x.shape[2]
            st, hyps = NR.crf_beam_search(x, init, beam, thr, stable=order == "stable")
            seen.add(st)
            try:
                seq, path = oracle.crf_beam_search(x, init, alphabet[:N], beam, thr)
            except RuntimeError as e:
                assert st != NR.OK and hyps == [], (st, str(e))
                continue
            assert st == NR.OK
            assert "".join(alphabet[l] for l in hyps[0][0]) == seq and hyps[0][1] == path
            assert len({tuple(h[0]) for h in hyps}) == len(hyps)
    assert {NR.OK, NR.BAD_STATE} <= seen, seen
