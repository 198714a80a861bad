"""TEST INFRASTRUCTURE: ragged, 16-bit and strided batches for the duplex searches (beam_search_duplex_batch_raw,
crf_beam_search_duplex_batch_raw).  Shared by tests/test_duplex_ragged_emu.py (CPU, emulated kernels, numpy inputs) and
tests/test_gpu_duplex_ragged.py.

Three kernels read the per-pair row counts, each with its own clamp -- env_width_kernel (its batch-wide maximum picks the
search kernel, the ring rows of a node and the staging), duplex_kernel (csrc/duplex.hip), duplex_slots_kernel
(csrc/duplex_slots.hip) -- and ln_convert_kernel is the only place that sees element types and strides.  The cases below
are the smallest at which each of them can go wrong.

Truth is ALWAYS the oracle with MATH_CR, called per pair on x1[i, :l1[i]] and x2[i, :l2[i]] with the envelope rows
[:l1[i]] and the pair's own init rows; for 16-bit inputs on the exact float32 upcast of what the kernel is given.  Strings
must be identical; a failing pair must carry the status whose status_string is the oracle's message (an input the
reference aborts on: FCD_ST_BAD_STATE) and out_len 0.  A pair with l1 == 0 has no oracle call -- the reference aborts on
envelope[(0, 1)] -- and must come back as FCD_ST_BAD_STATE.

Poison: what lies beyond a pair's own rows must never be used, so posterior rows >= l1[i] / >= l2[i] are NaN and envelope
rows >= l1[i] alternate between (2^40, 0) -- crossing bounds -- and (0, 2^40) -- a row as wide as read 2 if it counted.  The
oracle never sees the poison.

tall case    B = 4, T1cap = 12, T2cap = 600: see tall_case()
plain case   B = 8, T1cap = 48, T2cap = 52, N = 5, beam 5, threshold 0.05; an exact 1.0, an exact 0.0 and a float16
             subnormal planted in live rows of read 2
CRF case     B = 6, S = 4, N = 5, T1cap = 40, T2cap = 44; init arrays with S + 1 columns: pair 2's maximum sits in the extra
             column (a start state out of range), pair 1's init rows are all equal (the first maximum wins)
envelopes    1: band(l1[i], l2[i], 8) per pair   2: band(T1cap, T2cap, 10) for every pair (bounds above a pair's own T2 are
             clamped on later rows and fatal on row 0)   3: None (the default envelope ends at each pair's lengths_2)"""
import contextlib
import functools

import numpy as np

import test_gpu_duplex as D
from oracle import oracle

LSE, MAX, CR = D.LSE, D.MAX, D.CR
ALPHA = "NACGT"
MODES = (LSE, MAX)
FLAVOURS = (1, 2, 3)
POISON_ROWS = ((2 ** 40, 0), (0, 2 ** 40))
PANIC = oracle._MESSAGES[oracle.PANIC]
F32 = ("f32", "f32")


def _quantise(x, dtype):
    """float32 -> (the array handed to the library, its exact float32 upcast).  bfloat16 travels as uint16 bit patterns
    (truncation is enough for a test)."""
    if dtype == "f32":
        return x, x
    if dtype == "f16":
        h = x.astype(np.float16)
        return h, h.astype(np.float32)
    u = x.view(np.uint32) >> 16
    return u.astype(np.uint16), (u.astype(np.uint32) << 16).view(np.float32)


def _nan(dtype):
    return np.uint16(0x7FC0) if dtype == "bf16" else np.nan


class Case:
    def __init__(self, name, clean1, clean2, l1, l2, beam, thr, init1=None, init2=None):
        self.name, self.clean1, self.clean2 = name, clean1, clean2
        self.l1, self.l2 = np.asarray(l1, np.int64), np.asarray(l2, np.int64)
        self.B, self.T1, self.T2 = clean1.shape[0], clean1.shape[1], clean2.shape[1]
        self.crf = clean1.ndim == 4
        self.beam, self.thr, self.init1, self.init2 = beam, thr, init1, init2
        self._reads = {}

    def reads(self, dtypes=F32):
        """-> (q1, q2, up1, up2): the contiguous arrays in the element types handed over, poison in place, and the
        float32 upcasts of their CLEAN rows (what the oracle is given, pair by pair, up to the pair's lengths)"""
        if dtypes not in self._reads:
            out = []
            for clean, lens, dt in ((self.clean1, self.l1, dtypes[0]), (self.clean2, self.l2, dtypes[1])):
                q, up = _quantise(clean, dt)
                q = q.copy()
                for i, n in enumerate(lens):
                    q[i, n:] = _nan(dt)
                out.append((q, up))
            self._reads[dtypes] = (out[0][0], out[1][0], out[0][1], out[1][1])
        return self._reads[dtypes]


_CLEAR_LABEL = np.array([0.02, 0.9, 0.03, 0.03, 0.02], np.float32)


@functools.lru_cache(maxsize=None)
def plain_case(seed=9101):
    x1, x2 = D.pairs(seed, 8, 48, 52)
    x2[0, 20, 2] = 1.0               # probability one
    x2[5, 30, 0] = 0.0               # probability zero, in the blank column
    x2[6, 10, 3] = np.float32(6e-8)  # a float16 subnormal
    x1[1, 0] = x2[1, :3] = _CLEAR_LABEL  # (l1 = 1: a row that emits, so that the pair decodes to a non-empty string)
    return Case("plain", x1, x2, [48, 1, 0, 47, 33, 48, 17, 2], [52, 52, 30, 0, 1, 51, 20, 52], 5, 0.05)


@functools.lru_cache(maxsize=None)
def crf_case(seed=9200):
    B, S, N, T1, T2 = 6, 4, 5, 40, 44
    ps = [D.crf_pairs(seed + i, T1, T2, S, N) for i in range(B)]
    x1, x2 = np.stack([p[0] for p in ps]), np.stack([p[2] for p in ps])
    i1, i2 = np.zeros((B, S + 1), np.float32), np.zeros((B, S + 1), np.float32)
    for i, p in enumerate(ps):
        i1[i, :S], i2[i, :S] = p[1], p[3]
    x1[0, 0] = x2[0, :3] = _CLEAR_LABEL  # (l1 = 1: a row that emits)
    i1[1] = i2[1] = 0.25             # all-equal rows: the first maximum wins
    i1[2, S] = 2.0                   # the maximum in the extra column: a start state out of range
    # (three pairs fail by construction -- 2: init, 3: l2 = 0, 4: l1 = 0 -- so the other three must decode under every
    # flavour: l2 = 1, fatal on row 0 of flavour 2, goes with l1 = 0, and l1 - 8 < l2 keeps flavour 1's band valid)
    return Case("crf", x1, x2, [1, 40, 13, 25, 0, 39], [44, 43, 20, 0, 1, 35], 5, 0.05, i1, i2)


@functools.lru_cache(maxsize=None)
def tall_case(seed=9300):
    """The threshold between the two search kernels.  The slot-resident kernel keeps (beam * N + 1 + N) ring and tile rows
    of `ring rows` floats in 64 KiB of LDS (slds_words, csrc/duplex_slots.hip): 31 * ring rows words at beam 5, N 5, so
    a 600-row window cannot fit (31 * 604 > 16384) while the +-8 and +-10 bands do.  T2cap = 600 with short first reads:
    an envelope row beyond l1 that counted as T2 wide would push the whole batch off the slot-resident kernel -- which,
    forced, must refuse a launch only when a row of some PAIR is that wide."""
    x1, x2 = D.pairs(seed, 4, 12, 600)
    return Case("tall", x1, x2, [12, 4, 8, 0], [600, 600, 40, 600], 5, 0.05)


CASES = {"plain": plain_case, "crf": crf_case, "tall": tall_case}


def envelopes(case, flavour, wide=None):
    """(B, T1cap, 2) uint64 with the poison rows in place, or None for the default envelope.  `wide`: that pair gets the
    full matrix, (0, l2) on every one of its rows, instead."""
    if flavour == 3:
        return None
    env = np.empty((case.B, case.T1, 2), np.uint64)
    env[:, 0::2] = POISON_ROWS[0]
    env[:, 1::2] = POISON_ROWS[1]
    for i in range(case.B):
        n, m = int(case.l1[i]), int(case.l2[i])
        env[i, :n] = D.band(n, m, 8) if flavour == 1 else D.band(case.T1, case.T2, 10)[:n]
        if wide == i:
            env[i, :n] = (0, m)
    return env


def _oracle_pair(case, i, x1, x2, env, mode, collapse):
    """the oracle's outcome on one pair as handed in (a string: the consensus or the error's message) + its tie counters"""
    try:
        if case.crf:
            out = oracle.crf_beam_search_duplex(x1, case.init1[i], x2, case.init2[i], ALPHA, env, case.beam, case.thr, mode | CR)
        else:
            out = oracle.beam_search_duplex(x1, x2, ALPHA, env, case.beam, case.thr, collapse, mode | CR)
    except RuntimeError as err:
        out = str(err)
    return out, oracle.duplex_last_ambiguous()


@functools.lru_cache(maxsize=None)
def truth(name, flavour, mode, collapse=True, dtypes=F32, wide=None):
    """per pair (outcome, tie counters) of the oracle on the truncated pair; (None, (0, 0)) where l1 == 0"""
    case = CASES[name]()
    _, _, up1, up2 = case.reads(dtypes)
    env = envelopes(case, flavour, wide)
    out = []
    for i in range(case.B):
        n, m = int(case.l1[i]), int(case.l2[i])
        if n == 0:
            out.append((None, (0, 0)))
            continue
        out.append(_oracle_pair(case, i, up1[i, :n], up2[i, :m], None if env is None else env[i, :n], mode, collapse))
    return tuple(out)


def decoded(outcome):
    return outcome is not None and outcome not in oracle._MESSAGES.values()


def full_length_outcomes(name, flavour, mode, collapse=True):
    """{pair: outcome} of the oracle on the pairs with l1 > 0 and l2 < T2cap when read 2 keeps ALL its rows (clean rows
    stand in for the poison; flavour 2's rows are then not clamped, flavour 3's default envelope ends at T2cap)"""
    case = CASES[name]()
    _, _, up1, up2 = case.reads(F32)
    env = envelopes(case, flavour)
    out = {}
    for i in range(case.B):
        n = int(case.l1[i])
        if n > 0 and case.l2[i] < case.T2:
            out[i] = _oracle_pair(case, i, up1[i, :n], up2[i], None if env is None else env[i, :n], mode, collapse)[0]
    return out


def check_conditions(name, flavour, mode, collapse=True, dtypes=F32, wide=None):
    """a launch cannot pass vacuously: at least half of its pairs decode to a non-empty string and at least one fails"""
    t = truth(name, flavour, mode, collapse, dtypes, wide)
    good = sum(1 for w, _ in t if decoded(w) and len(w) > 0)
    bad = sum(1 for w, _ in t if not decoded(w))
    assert 2 * good >= len(t) and bad >= 1, (name, flavour, mode, collapse, dtypes, [w for w, _ in t])


def check_lengths_matter(name, flavour, mode):
    """at least three pairs with l2 < T2cap whose outcome changes when read 2 keeps all its rows, at least one of them
    from one consensus to another: a kernel that ignored lengths_2 is caught.  (Flavour 2 is where a kernel's own clamp
    to lengths_2 decides anything: flavour 1's bounds end at l2[i] by construction and flavour 3's envelope is made from
    lengths_2 on the host, so there a search kernel that ignored lengths_2 would compute the same.  The seeds of the two
    cases were chosen for this condition; of 100 seeds about half give it in both modes.)"""
    t = truth(name, flavour, mode)
    full = full_length_outcomes(name, flavour, mode)
    differ = [i for i, w in full.items() if w != t[i][0]]
    strings = [i for i in differ if decoded(full[i]) and decoded(t[i][0])]
    assert len(differ) >= 3 and len(strings) >= 1, (name, flavour, mode, differ, strings)


# ---- what the library is handed -------------------------------------------------------------------------------------
def _to_device(a, dtype, device):
    import torch
    if dtype == "bf16":
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(device).view(torch.bfloat16)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _strided_big(q, dtype):
    """a (B, 2 * Tcap, 8) array of NaNs holding q in [:, ::2, 1:6]"""
    assert q.ndim == 3 and q.shape[2] == 5
    big = np.full((q.shape[0], 2 * q.shape[1], 8), _nan(dtype), q.dtype)
    big[:, ::2, 1:6] = q
    return big


def handed(q, dtype, layout, device=None):
    """q, contiguous (B, T, ...), in the storage `layout` names: "batch" as it is, "time" a (T, B, ...) array handed over
    as .transpose(1, 0, ...), "view" the column and row view big[:, ::2, 1:6] -- as a numpy array or on `device`"""
    if device is None:
        if dtype == "bf16":
            raise TypeError("the host entries of the duplex searches take float32 and float16")
        if layout == "time":
            return np.ascontiguousarray(np.swapaxes(q, 0, 1)).swapaxes(0, 1)
        return _strided_big(q, dtype)[:, ::2, 1:6] if layout == "view" else q
    if layout == "view":
        return _to_device(_strided_big(q, dtype), dtype, device)[:, ::2, 1:6]
    t = _to_device(q, dtype, device)
    return t.transpose(0, 1).contiguous().transpose(0, 1) if layout == "time" else t


class _Ragged:
    """the module as D.gpu_strings sees it: every launch carries the case's lengths, the last result is kept"""

    def __init__(self, fcd, case, **kw):
        self.fcd, self.api, self.case, self.kw, self.last = fcd, fcd.api, case, kw, None

    def beam_search_duplex_batch_raw(self, *a, **k):
        self.last = self.fcd.beam_search_duplex_batch_raw(*a, lengths_1=self.case.l1, lengths_2=self.case.l2, **self.kw, **k).cpu()
        return self.last

    def crf_beam_search_duplex_batch_raw(self, *a, **k):
        self.last = self.fcd.crf_beam_search_duplex_batch_raw(*a, lengths_1=self.case.l1, lengths_2=self.case.l2, **self.kw, **k).cpu()
        return self.last


def crf_gpu_strings(fcd, x1, i1, x2, i2, alpha, envs, beam, thr, mode):
    """D.gpu_strings for the CRF search (labels come leaf -> root: src/duplex.rs:825-833)"""
    r = fcd.crf_beam_search_duplex_batch_raw(x1, i1, x2, i2, envs, beam, thr, logadd_mode=mode).cpu()
    out = []
    for i in range(x1.shape[0]):
        if int(r.status[i]) != 0:
            out.append(fcd.api.nat.status_string(int(r.status[i])))
        else:
            out.append("".join(alpha[l] for l in r.labels[i, :int(r.out_len[i])][::-1])[::-1])
    return out


def expected_strings(fcd, t):
    aborts = fcd.api.nat.status_string(fcd.api.nat.ST_BAD_STATE)
    return [aborts if (w is None or w == PANIC) else w for w, _ in t]


def run(fcd, name, flavour, mode, collapse=True, dtypes=F32, layouts=("batch", "batch"), device=None, wide=None,
        count_ambiguous=False, envs="flavour"):
    """one launch of the case against the oracle -> the result (host arrays).  `envs`: an envelope array (or device
    tensor) to hand over instead of the flavour's own -- the truth is then the caller's business and nothing is compared."""
    case = CASES[name]()
    q1, q2, _, _ = case.reads(dtypes)
    a1, a2 = handed(q1, dtypes[0], layouts[0], device), handed(q2, dtypes[1], layouts[1], device)
    own = isinstance(envs, str)
    env = envelopes(case, flavour, wide) if own else envs
    shim = _Ragged(fcd, case, count_ambiguous=count_ambiguous)
    if case.crf:
        got = crf_gpu_strings(shim, a1, case.init1, a2, case.init2, ALPHA, env, case.beam, case.thr, mode)
    else:
        got = D.gpu_strings(shim, a1, a2, ALPHA, env, case.beam, case.thr, collapse, mode)
    r = shim.last
    r.strings = got
    if not own:
        return r
    t = truth(name, flavour, mode, collapse, dtypes, wide)
    what = (name, flavour, mode, collapse, dtypes, layouts, "device" if device is not None else "host", wide)
    assert got == expected_strings(fcd, t), (what, got, expected_strings(fcd, t))
    for i, (w, amb) in enumerate(t):
        if not decoded(w):
            assert int(r.status[i]) != 0 and int(r.out_len[i]) == 0, (what, i)
        if count_ambiguous:
            assert tuple(int(v) for v in r.ambiguous[i]) == amb, (what, i, r.ambiguous[i], amb)
    return r


def same(a, b, pairs=None):
    """two results agree on `pairs` (default: all): status, out_len, the labels up to out_len, the tie counters"""
    for i in (range(len(a.out_len)) if pairs is None else pairs):
        n = int(a.out_len[i])
        assert int(a.status[i]) == int(b.status[i]) and int(b.out_len[i]) == n, i
        assert np.array_equal(np.asarray(a.labels[i, :n]), np.asarray(b.labels[i, :n])), i
        if a.ambiguous is not None and b.ambiguous is not None:
            assert np.array_equal(np.asarray(a.ambiguous[i]), np.asarray(b.ambiguous[i])), i


@contextlib.contextmanager
def forced_kernel(which):
    """0: AUTO, 1: the any-shape kernel (csrc/duplex.hip), 2: the slot-resident one (csrc/duplex_slots.hip)"""
    from fast_ctc_decode_amd import _native as nat
    h = nat.default_handle()
    assert h.lib.fcd_debug_set_duplex_kernel(h.ptr, which) == 0
    try:
        yield h
    finally:
        assert h.lib.fcd_debug_set_duplex_kernel(h.ptr, 0) == 0


# ---- the launch whose widest row belongs to ONE pair, and the same launch in chunks -----------------------------------
WIDE_PAIR = 5  # l1 = 48, l2 = 51: (0, 51) on every row, the batch's ring size and staging follow from it


def chunk_limit(case, which, width):
    """a workspace limit under which duplex_dev (csrc/capi.hip) decodes the case three pairs at a time: chunk =
    limit / per_pair with, for the plain case (T1cap 48, T2cap 52, beam 5, N 5, NL 4) and width 51,
      cap_nodes = (T1cap * beam * NL + 8 + 3) & ~3 = 968
      slot-resident kernel (AUTO, 2): ring rows = (width + 4 + 3) & ~3 = 56,
          per_pair = (cap_nodes * (32 + ring * 4 + NLp * 4) + (T2cap + 1) * 4 + 255) & ~255 = 263680
      any-shape kernel (1): Wcap = width + 2 = 53,
          per_pair = cap_nodes * (16 + 8 + NL * 4 + Wcap * 12) + (((T2cap + 1) * 4 + 64 + 15) & ~15) = 654656
    limit = 3.5 * per_pair: 8 pairs go in chunks of 3, 3 and 2."""
    NL = 4
    cap_nodes = (case.T1 * case.beam * NL + 8 + 3) & ~3
    if which == 1:
        per_pair = cap_nodes * (16 + 8 + NL * 4 + (width + 2) * 12) + (((case.T2 + 1) * 4 + 64 + 15) & ~15)
    else:
        ring = (width + 4 + 3) & ~3
        per_pair = (cap_nodes * (32 + ring * 4 + 4 * 4) + (case.T2 + 1) * 4 + 255) & ~255
    limit = 3 * per_pair + per_pair // 2
    assert limit // per_pair == 3
    return limit


# ---- the band estimator in the loop ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def estimator_truth(mode, band=8):
    """per pair of the plain case with l1 > 0: (the envelope tests/envelope_model.py gives for the truncated pair from
    the oracle's greedy decodes of its two reads, the oracle's outcome of the search inside it)"""
    import envelope_model as em
    case = plain_case()
    _, _, up1, up2 = case.reads()
    out = []
    for i in range(case.B):
        n, m = int(case.l1[i]), int(case.l2[i])
        if n == 0:
            out.append((None, None))
            continue
        lab1, path1, _ = oracle.viterbi_search_raw(np.ascontiguousarray(up1[i, :n]))
        lab2, path2 = ([], []) if m == 0 else oracle.viterbi_search_raw(np.ascontiguousarray(up2[i, :m]))[:2]
        env = em.envelope(lab1, path1, n, lab2, path2, m, band)
        out.append((env, _oracle_pair(case, i, up1[i, :n], up2[i, :m], env, mode, True)[0]))
    return tuple(out)


def estimator_loop(fcd, mode, device=None, band=8):
    """estimate_envelope_batch on the ragged plain case with the poison in place, its result handed straight to the
    search with the same lengths: envelope rows [:l1] equal the model's, every pair equals the oracle inside them"""
    case = plain_case()
    q1, q2, _, _ = case.reads()
    a1, a2 = handed(q1, "f32", "batch", device), handed(q2, "f32", "batch", device)
    env = fcd.estimate_envelope_batch(a1, a2, band, case.l1, case.l2)
    r = run(fcd, "plain", None, mode, device=device, envs=env)
    env = env if isinstance(env, np.ndarray) else env.cpu().numpy().view(np.uint64)
    t = estimator_truth(mode, band)
    aborts = fcd.api.nat.status_string(fcd.api.nat.ST_BAD_STATE)
    assert sum(1 for _, w in t if decoded(w) and len(w) > 0) >= case.B // 2
    for i, (want_env, w) in enumerate(t):
        if want_env is not None:
            np.testing.assert_array_equal(env[i, :case.l1[i]], want_env, err_msg="pair %d" % i)
        assert r.strings[i] == (aborts if (w is None or w == PANIC) else w), (mode, i, r.strings[i], w)
        if not decoded(w):
            assert int(r.out_len[i]) == 0, i
    return r
