"""TEST INFRASTRUCTURE: the beam-search session case matrix shared by tests/test_session_emu.py (CPU, emulated kernels)
and tests/test_gpu_session.py (MI355X).  Every kernel family a session runs on, plain and CRF: random chunkings (1-row
pushes, 0-row slots, ragged per-slot lengths), the result after EVERY push against the oracle on each slot's prefix and
the final one against the one-shot batch call on the concatenation, push(result=True) against push + result(), a NaN in
a later chunk, a threshold that runs out of beam, a NaN CRF init row, restarts, refused over-long pushes, f16 and
time-major chunks."""
import numpy as np

from oracle import oracle

KERNEL_AUTO, KERNEL_GENERIC, KERNEL_WAVE, KERNEL_WAVE1, KERNEL_LANE = 0, 1, 2, 3, 4
OK, BAD_STATE = 0, 4  # (the oracle's PANIC is the library's FCD_ST_BAD_STATE)

# (N, beam, kernel): wave RPW 2, wave RPW 1 (groups of eight and of five), generic, and beam 32 on AUTO (lands on generic)
PLAIN = [(5, 5, KERNEL_WAVE), (7, 8, KERNEL_WAVE1), (5, 12, KERNEL_WAVE), (12, 5, KERNEL_GENERIC), (5, 32, KERNEL_AUTO)]
# (N, S, beam, kernel): CRF wave with the register FIFO (S 4) and the row gather (S 64), CRF generic
CRF = [(5, 4, 5, KERNEL_WAVE), (5, 64, 5, KERNEL_WAVE), (4, 3, 5, KERNEL_GENERIC)]


def plain_batch(seed, N, T=60, B=6):
    rng = np.random.default_rng(seed)
    x = rng.random((B, T, N), dtype=np.float32)
    x[1] = (rng.integers(1, 4, size=(T, N)) / 4.0).astype(np.float32)  # ties
    z = rng.normal(size=(T, N)).astype(np.float32) * 4.0
    x[2] = np.exp(z - z.max(-1, keepdims=True))                         # peaky
    x /= x.sum(-1, keepdims=True)
    x[4, 2 * T // 3, 1] = np.nan                                       # IncomparableValues in a later chunk
    return x.astype(np.float32)


def crf_batch(seed, N, S, T=48, B=5):
    rng = np.random.default_rng(seed)
    x = rng.random((B, T, S, N), dtype=np.float32)
    x[1] = (rng.integers(1, 4, size=(T, S, N)) / 4.0).astype(np.float32)
    x[3, T // 2] = np.nan
    init = rng.random((B, S), dtype=np.float32)
    init[4, 1] = np.nan  # a NaN init row: BadState at the slot's first non-empty push
    return x, init


def chunkings(rng, B, T):
    """per push, per slot row counts: 1-row pushes, 0-row slots, ragged lengths; every slot ends at T rows"""
    done = np.zeros(B, np.int64)
    pushes = []
    k = 0
    while (done < T).any():
        if k < 2:
            take = np.full(B, 1, np.int64)       # 1-row pushes first
        else:
            take = rng.integers(0, 12, size=B)   # ragged, with 0-row slots
        take = np.minimum(take, T - done)
        pushes.append(take)
        done += take
        k += 1
    return pushes


def want_plain(x, beam, thr, collapse):
    """the oracle on a prefix: (status, labels, path, (the two tie counters))"""
    return oracle.beam_search_ambiguous(np.ascontiguousarray(x), beam, thr, collapse)


def want_crf(x, init, beam, thr):
    st, labels, path, amb = oracle.crf_beam_search_ambiguous(np.ascontiguousarray(x), np.ascontiguousarray(init), beam, thr)
    return (BAD_STATE if st == oracle.PANIC else st), labels, path, amb


def check_slot(r, i, want, what=""):
    """status, labels, path, out_len -- and the tie counters where the result carries them (count_ambiguous sessions)"""
    st, labels, path, amb = want
    assert int(r.status[i]) == st, (what, i, int(r.status[i]), st)
    if r.ambiguous is not None and st != BAD_STATE:  # (the oracle panics there: it counts nothing)
        got = tuple(int(v) for v in np.asarray(r.ambiguous[i]))
        assert got == tuple(amb), (what, i, got, amb)
    if st != OK:
        assert int(r.out_len[i]) == 0, (what, i)
        return
    n = int(r.out_len[i])
    assert n == len(labels), (what, i, n, len(labels))
    assert np.array_equal(np.asarray(r.labels[i, :n]).astype(np.int64), np.asarray(labels).astype(np.int64)), (what, i)
    assert np.array_equal(np.asarray(r.path[i, :n]).astype(np.int64), np.asarray(path).astype(np.int64)), (what, i)


def same_result(a, b, what=""):
    for i in range(len(a.out_len)):
        assert int(a.status[i]) == int(b.status[i]), (what, i)
        n = int(a.out_len[i])
        assert n == int(b.out_len[i]), (what, i)
        assert np.array_equal(np.asarray(a.labels[i, :n]), np.asarray(b.labels[i, :n])), (what, i)
        assert np.array_equal(np.asarray(a.path[i, :n]).astype(np.int64), np.asarray(b.path[i, :n]).astype(np.int64)), (what, i)
    if a.ambiguous is not None or b.ambiguous is not None:
        assert np.array_equal(np.asarray(a.ambiguous).astype(np.int64), np.asarray(b.ambiguous).astype(np.int64)), what


def _slices(x, pushes):
    """the chunks of a chunking: chunk k holds, for slot i, rows [done_i, done_i + take_i) at its start"""
    B = x.shape[0]
    done = np.zeros(B, np.int64)
    for take in pushes:
        Tc = max(int(take.max()), 1)
        c = np.zeros((B, Tc) + x.shape[2:], x.dtype)
        for i in range(B):
            c[i, :take[i]] = x[i, done[i]:done[i] + take[i]]
        yield c, take, done.copy()
        done += take


def run_plain(fcd, N, beam, kernel, seed=0, thr=0.0, collapse=True, to_input=None, every=True, host=True):
    """pushes a random chunking through a session; after every push (every=True) each slot's result equals the oracle on
    its prefix; at the end the result equals beam_search_batch_raw on the whole reads (ambiguous counters included)"""
    x = plain_batch(100 + seed + N * 7 + beam, N)
    B, T = x.shape[:2]
    rng = np.random.default_rng(seed)
    pushes = chunkings(rng, B, T)
    conv = to_input or (lambda a: a)
    with fcd.BeamSearchSession(B, N, T, beam, thr, collapse, count_ambiguous=True, kernel=kernel) as s:
        for k, (c, take, done) in enumerate(_slices(x, pushes)):
            use_result = k % 2 == 0
            r = s.push(conv(c), take, result=use_result)
            if use_result:
                same_result(r.cpu(), s.result(host=host).cpu(), "push(result=True) vs result()")
            if every:
                r = s.result(host=host).cpu()
                for i in range(B):
                    check_slot(r, i, want_plain(x[i, :done[i] + take[i]], beam, thr, collapse), "push %d" % k)
        assert (s.steps == T).all()
        final = s.result(host=host).cpu()
    one = fcd.beam_search_batch_raw(x, beam, thr, collapse, kernel=kernel, count_ambiguous=True).cpu()
    same_result(final, one, "final vs one-shot")
    return final


def run_crf(fcd, N, S, beam, kernel, seed=0, thr=0.0, to_input=None, every=True, host=True):
    x, init = crf_batch(200 + seed + N + S + beam, N, S)
    B, T = x.shape[:2]
    rng = np.random.default_rng(seed + 5)
    pushes = chunkings(rng, B, T)
    conv = to_input or (lambda a: a)
    with fcd.CrfBeamSearchSession(B, S, N, init, T, beam, thr, count_ambiguous=True, kernel=kernel) as s:
        r0 = s.result(host=host).cpu()  # before the first push: reads of length 0 (a bad init row too)
        assert (np.asarray(r0.status) == OK).all() and (np.asarray(r0.out_len) == 0).all()
        for k, (c, take, done) in enumerate(_slices(x, pushes)):
            r = s.push(conv(c), take, result=True)
            if every:
                r = r.cpu()
                for i in range(B):
                    check_slot(r, i, want_crf(x[i, :done[i] + take[i]], init[i], beam, thr), "push %d" % k)
        final = s.result(host=host).cpu()
    one = fcd.crf_beam_search_batch_raw(x, init, beam, thr, kernel=kernel, count_ambiguous=True).cpu()
    same_result(final, one, "final vs one-shot")
    assert int(final.status[4]) == BAD_STATE  #: the NaN init row
    return final


def run_out_of_beam(fcd, N, beam, kernel, host=True):
    """a threshold no label passes on a row whose blank is below it too, in a later chunk: RanOutOfBeam from that push on"""
    x = plain_batch(77 + N + beam, N)
    x[0, 40] = 0.01
    B, T = x.shape[:2]
    with fcd.BeamSearchSession(B, N, T, beam, 0.05, kernel=kernel) as s:
        s.push(x[:, :30])
        r = s.result(host=host).cpu()
        assert int(r.status[0]) == OK
        s.push(x[:, 30:])
        r = s.result(host=host).cpu()
    for i in range(B):
        check_slot(r, i, want_plain(x[i], beam, 0.05, True), "out of beam")
    assert int(r.status[0]) == 1


def run_restart(fcd, N, beam, kernel, host=True):
    """restarting some slots half way equals a fresh session for them and leaves the others untouched"""
    x = plain_batch(5 + N + beam, N)
    y = plain_batch(6 + N + beam, N)
    B, T = x.shape[:2]
    with fcd.BeamSearchSession(B, N, 2 * T, beam, 0.0, kernel=kernel) as s:
        s.push(x[:, :25])
        s.restart([1, 3])
        st = s.steps
        assert st[1] == 0 and st[3] == 0 and st[0] == 25
        c = x[:, 25:].copy()
        c[1], c[3] = y[1, :T - 25], y[3, :T - 25]
        s.push(c)
        r = s.result(host=host).cpu()
    for i in range(B):
        want = want_plain(y[i, :T - 25], beam, 0.0, True) if i in (1, 3) else want_plain(x[i], beam, 0.0, True)
        check_slot(r, i, want, "restart")


def run_crf_restart(fcd, N, S, beam, kernel, host=True):
    x, init = crf_batch(9 + S, N, S)
    B, T = x.shape[:2]
    init2 = np.random.default_rng(3).random((2, S), dtype=np.float32)
    with fcd.CrfBeamSearchSession(B, S, N, init, T, beam, 0.0, kernel=kernel) as s:
        s.push(x[:, :20])
        s.restart([4, 0], init2)  # slot 4's NaN init row is replaced before it ever ran
        c = np.zeros_like(x[:, :T - 20])
        c[:] = x[:, 20:]
        s.push(c, lengths=[T - 20, T - 20, T - 20, T - 20, T - 20])
        r = s.result(host=host).cpu()
    for i in range(B):
        if i in (0, 4):
            want = want_crf(x[i, 20:], init2[1 if i == 0 else 0], beam, 0.0)
        else:
            want = want_crf(x[i], init[i], beam, 0.0)
        check_slot(r, i, want, "crf restart")


def run_refused(fcd, N, beam, kernel, host=True):
    """a push past max_steps is refused before anything runs: results and step counts unchanged"""
    import pytest
    x = plain_batch(11, N)
    B = x.shape[0]
    with fcd.BeamSearchSession(B, N, 40, beam, 0.0, kernel=kernel) as s:
        s.push(x[:, :30])
        before = s.result(host=host).cpu()
        with pytest.raises(ValueError, match="max_steps"):
            s.push(x[:, 30:41])
        with pytest.raises(ValueError, match="max_steps"):
            s.push(x[:, 30:50], lengths=[5, 5, 5, 15, 5, 5])
        assert (s.steps == 30).all()
        same_result(s.result(host=host).cpu(), before, "refused push")
        s.push(x[:, 30:40])  # exactly max_steps: accepted
        assert (s.steps == 40).all()
