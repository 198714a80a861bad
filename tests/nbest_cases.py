"""TEST INFRASTRUCTURE: the n-best case matrix shared by tests/test_nbest_emu.py (CPU, emulated kernels) and
tests/test_gpu_nbest.py (MI355X): every kernel family, plain and CRF, on small shapes with ragged lengths (0 and 1
included), a NaN read and a threshold that runs out of beam; every hypothesis against tests/nbest_reference.py, and
hypothesis 0 against the existing single-result call."""
import numpy as np

import nbest_reference as NR

KERNEL_AUTO, KERNEL_GENERIC, KERNEL_WAVE, KERNEL_WAVE1, KERNEL_LANE = 0, 1, 2, 3, 4

# (N, beam, kernel): wave RPW 2, wave RPW 1 (groups of eight and of five), lane, generic
PLAIN = [(5, 5, KERNEL_WAVE), (7, 8, KERNEL_WAVE1), (5, 12, KERNEL_WAVE), (5, 32, KERNEL_LANE), (8, 13, KERNEL_LANE),
         (12, 5, KERNEL_GENERIC)]
# (N, S, beam, kernel)
CRF = [(5, 4, 5, KERNEL_WAVE), (5, 64, 5, KERNEL_WAVE), (5, 4, 16, KERNEL_LANE), (4, 3, 5, KERNEL_GENERIC)]


def plain_batch(seed, N, T=48):
    rng = np.random.default_rng(seed)
    x = rng.random((7, T, N), dtype=np.float32)
    x[1] = (rng.integers(1, 4, size=(T, N)) / 4.0).astype(np.float32)  # ties
    z = rng.normal(size=(T, N)).astype(np.float32) * 4.0
    x[2] = np.exp(z - z.max(-1, keepdims=True))                         # peaky
    x /= x.sum(-1, keepdims=True)
    x[5, T // 2, 1] = np.nan                                           # IncomparableValues half way
    lengths = np.array([T, T, T - 3, 0, 1, T, T], np.int64)
    return x.astype(np.float32), lengths


def crf_batch(seed, N, S, T=40):
    rng = np.random.default_rng(seed)
    x = rng.random((5, T, S, N), dtype=np.float32)
    x[1] = (rng.integers(1, 4, size=(T, S, N)) / 4.0).astype(np.float32)
    x[4, T // 3] = np.nan
    init = rng.random((5, S), dtype=np.float32)
    lengths = np.array([T, T, 1, 0, T], np.int64)
    return x, init, lengths


def check(r, want, n_best, B):
    """r: a (cpu) NBestResult; want: per read (status, hypotheses) of tests/nbest_reference.py"""
    for i in range(B):
        st, hyps = want[i]
        assert int(r.status[i]) == st, (i, int(r.status[i]), st)
        n_hyp = min(n_best, len(hyps)) if st == NR.OK else 0
        assert int(r.n_hyp[i]) == n_hyp, (i, int(r.n_hyp[i]), n_hyp)
        for j in range(n_best):
            n = int(r.out_len[i, j])
            if j >= n_hyp:
                assert n == 0 and float(r.score[i, j]) == 0.0, (i, j)
                continue
            labels, path, score = hyps[j]
            assert n == len(labels), (i, j, n, len(labels))
            assert r.labels[i, j, :n].tolist() == labels, (i, j)
            assert r.path[i, j, :n].tolist() == path, (i, j)
            got = np.float32(r.score[i, j])
            assert got.tobytes() == np.float32(score).tobytes(), (i, j, got, score)  # bit-exact


def check_hyp0(r, single, B):
    """hypothesis 0 of every read equals the single-result call (a cpu BatchResult), byte for byte"""
    for i in range(B):
        assert int(r.status[i]) == int(single.status[i]), i
        if int(single.status[i]) != 0:
            continue
        n = int(single.out_len[i])
        assert int(r.out_len[i, 0]) == n, i
        assert np.array_equal(np.asarray(r.labels[i, 0, :n]), np.asarray(single.labels[i, :n])), i
        assert np.array_equal(np.asarray(r.path[i, 0, :n]).astype(np.int64), np.asarray(single.path[i, :n]).astype(np.int64)), i


def run_plain(fcd, N, beam, kernel, stable, seed=0, thr=0.0, n_best=None, to_input=None):
    x, lengths = plain_batch(1000 + seed + N * 7 + beam, N)
    n_best = beam if n_best is None else n_best
    xin = x if to_input is None else to_input(x)
    r = fcd.beam_search_nbest_batch_raw(xin, n_best, beam, thr, lengths=lengths, kernel=kernel).cpu()
    want = [NR.beam_search(x[i, :lengths[i]], beam, thr, True, stable=stable) for i in range(x.shape[0])]
    check(r, want, n_best, x.shape[0])
    single = fcd.beam_search_batch_raw(xin, beam, thr, lengths=lengths, kernel=kernel).cpu()
    check_hyp0(r, single, x.shape[0])
    return r


def run_crf(fcd, N, S, beam, kernel, stable, seed=0, thr=0.0, n_best=None, to_input=None):
    x, init, lengths = crf_batch(2000 + seed + N + S + beam, N, S)
    n_best = beam if n_best is None else n_best
    xin = x if to_input is None else to_input(x)
    r = fcd.crf_beam_search_nbest_batch_raw(xin, init, n_best, beam, thr, lengths=lengths, kernel=kernel).cpu()
    want = [NR.crf_beam_search(x[i, :lengths[i]], init[i], beam, thr, stable=stable) for i in range(x.shape[0])]
    check(r, want, n_best, x.shape[0])
    single = fcd.crf_beam_search_batch_raw(xin, init, beam, thr, lengths=lengths, kernel=kernel).cpu()
    check_hyp0(r, single, x.shape[0])
    return r


def run_out_of_beam(fcd, N, beam, kernel):
    """a threshold no label passes on rows whose blank is below it too: RanOutOfBeam, n_hyp 0, every row empty"""
    x, lengths = plain_batch(77 + N + beam, N)
    x[0, 10] = 0.01
    x[6, 20] = 0.01
    r = fcd.beam_search_nbest_batch_raw(x, beam, beam, 0.05, lengths=lengths, kernel=kernel).cpu()
    want = [NR.beam_search(x[i, :lengths[i]], beam, 0.05, True) for i in range(x.shape[0])]
    assert want[0][0] == NR.RAN_OUT_OF_BEAM and want[6][0] == NR.RAN_OUT_OF_BEAM
    check(r, want, beam, x.shape[0])
