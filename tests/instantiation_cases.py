"""TEST INFRASTRUCTURE: the instantiation ledger -- for EVERY kernel instantiation the library compiles, one small call
that makes the host dispatch choose exactly that instantiation, and its check against the reference.

The dispatchers multiply N x lane group x reads per wavefront x S x AMB x UNI x H16 x PDQ x NB x SES (csrc/beam_wave.hip,
beam_wave_session.hip, beam_lane.hip), dtype x N (viterbi.hip), chain x states per lane (crf_posterior.hip) ...: every
product is separately compiled code with its own `if constexpr` arms and its own register allocation, and the
feature-by-feature case tables reach a fraction of them.  Here every family has ONE function from a template-argument
tuple to a call (`FAMILIES`), and `rows()` enumerates the tuples the dispatchers can choose.

    tests/test_instantiation_ledger_emu.py   (CPU)  the compiled set (nm on libfcd_emu.so, and the gfx950 code objects
                                             of libfcd_hip.so) == rows() + EXEMPT; every row, run on the emulator, launches
                                             exactly its instantiation (the emulator's launch log) and passes its check
    tests/test_gpu_instantiations.py         (GPU)  the same rows on the device, grouped by family

Shapes: the smallest at which these kernels can go wrong.  B = 3 (an odd count: one half-wave without a read); T from
{1, 7, 65, 130} (below, at and past the six-row FIFO block and the 64-deep traceback segments): every row runs one short
and one long T, taken in turn; lengths (T, T - 3, 0) where UNI = false and none where UNI = true; read 0 is quantised
(rank32_cases.quantised: rows of k / 4, so equal probabilities exist and -- where a shape holds more than 20 candidates
-- the two tie orders differ), read 1 has values of k / 256 (exact in binary16 and bfloat16), read 2 is peaky; f16 AND
bf16 inputs for every H16 instantiation (the n-best ones, whose H16 is on whatever the input, and the lane and generic
kernels, which take the element type at run time, get float32 as well); count_ambiguous for AMB, checked against the oracle's counters (rank32_cases.counted's source).
The searches are compared exactly (session_cases.check_slot, nbest_cases.check); the lattice kernels keep the tolerances
of their case files.

The GPU cannot say which kernel ran, so the GPU twin relies on the emulator build choosing as the device build does.
Every FCD_HIPEMU branch under csrc/:
  inside device code or declarations, where no launch is decided -- plain-C++ forms of instructions (device_utils.h:111,
  :188, :200; duplex_math.h:122; duplex_slots.hip:142; crf_transitions.hip:30), the LDS address-space qualifier (pdq178_reg.h:30, :50;
  pdq178_wave.h:53, :59), <stdio.h> for the kernels' abort messages (beam_wave.hip:49, beam_lane.hip:29), the emulator's
  pass counters (duplex_slots.hip:183, :1129), the LDS-DMA prefetch left out (duplex_slots.hip:798), LDS and device memory
  made garbage as on the GPU (beam_lane.hip:179, :932; beam_wave_step.inc:643), the all-pairs switch of the lane kernel's
  node order (beam_lane.hip:690);
  in host code --
    ctc_score.hip:231, ctc_align.hip:421, fcd_internal.h:150 (allow_dynamic_lds)
                                           hipFuncSetAttribute for more than 64 KiB of dynamic LDS is skipped: the launch
                                           that follows is the same kernel;
    tieorder.hip:68, beam_lane.hip:1113    the cycle counters of the profiling builds read back as zeros (fcd_debug.h);
    duplex_slots.hip:1508                  a statistics line on stderr after the launch;
    beam_lane.hip:1157                     beam_lane_resident_waves returns 3: it sizes the slab pool of the two-pass
                                           path (capi.hip beam_dev, p1 / p2), never the instantiation -- launch_nap takes
                                           RPW from beam_size and the retry counter alone;
    slab_pool.h:29, glibc235_math.h:30     `__HIPCC__ || FCD_HIPEMU`: the same code for both.
None of them changes which instantiation is chosen."""
import math
import re

import numpy as np

import nbest_cases as NC
import nbest_reference as NR
import rank32_cases as RC
import session_cases as SC
from oracle import oracle
from tie_util import tie_order

KERNEL_AUTO, KERNEL_GENERIC, KERNEL_WAVE, KERNEL_WAVE1, KERNEL_LANE = 0, 1, 2, 3, 4
TS = (1, 7, 65, 130)
B = 3


# ---- names -----------------------------------------------------------------------------------------------------------
def canonical(name):
    """`void fcd::(anonymous namespace)::k<5, 6, true>(fcd::P)` (nm -C, llvm-cxxfilt) and
    `const char* hipemu::kname<fcd::{anonymous}::k<5, 6, true> >()` (the launch log) -> `k<5,6,true>`"""
    s = name.strip()
    m = re.match(r"^const char\s*\*\s*hipemu::kname<&?\(?(.*?)\)?\s*>\(\)$", s)
    if m:
        s = m.group(1)
    s = re.sub(r"^void\s+", "", s)
    s = s.replace("(anonymous namespace)::", "").replace("{anonymous}::", "").replace("fcd::", "")
    depth, end = 0, len(s)
    for i, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            end = i
            break
    s = s[:end].replace(" ", "")
    return re.sub(r"\((?:bool|int|unsigned|[A-Za-z_:]+)\)(-?\d+)", r"\1", s)  # (a cast spelt out: `(int)2`)


def parse(canon):
    """`k<5,6,true>` -> ("k", (5, 6, True)); `k` -> ("k", ())"""
    m = re.match(r"^(\w+)(?:<(.*)>)?$", canon)
    assert m, canon
    args = tuple(a == "true" if a in ("true", "false") else int(a) for a in (m.group(2).split(",") if m.group(2) else ()))
    return m.group(1), args


def spell(template, args):
    if not args:
        return template
    return "%s<%s>" % (template, ",".join(("true" if a else "false") if isinstance(a, bool) else str(a) for a in args))


# ---- inputs ----------------------------------------------------------------------------------------------------------
def ts_of(key):
    """one short and one long T for a row, taken in turn over the rows of a family"""
    k = sum(int(v) * (i + 3) for i, v in enumerate(key) if not isinstance(v, str))
    return (TS[k % 2], TS[2 + (k // 2) % 2])


def plain_reads(N, T, seed):
    """(3, T, N) float32, every value exact in binary16 and bfloat16: quantised, k / 256, peaky"""
    rng = np.random.default_rng(seed)
    x = np.empty((B, T, N), np.float32)
    x[0] = RC.quantised(seed, T) if N == RC.N else (rng.integers(1, 4, size=(T, N)) / 4.0)
    x[1] = rng.integers(1, 257, size=(T, N)) / 256.0
    x[2] = rng.integers(1, 9, size=(T, N)) / 256.0
    x[2, np.arange(T), rng.integers(0, N, size=T)] = 0.75
    return x


def crf_reads(S, T, seed, N=5):
    rng = np.random.default_rng(seed)
    x = np.empty((B, T, S, N), np.float32)
    x[0] = rng.integers(1, 4, size=(T, S, N)) / 4.0
    x[1] = rng.integers(1, 257, size=(T, S, N)) / 256.0
    x[2] = rng.integers(1, 9, size=(T, S, N)) / 256.0
    x[2, :, :, 0] = 0.5
    x[2, np.arange(T), :, rng.integers(0, N, size=T)] = 0.75
    init = (rng.integers(1, 9, size=(B, S)) / 8.0).astype(np.float32)
    return x, init


def bf16_bits(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    assert not (b & 0xFFFF).any(), "not exact in bfloat16"
    return (b >> 16).astype(np.uint16)


def f16(x):
    h = x.astype(np.float16)
    assert np.array_equal(h.astype(np.float32), x), "not exact in binary16"
    return h


def inputs_of(x, h16, f32=False):
    """(array, input_dtype) forms a row feeds: float32, or both 16-bit types (f32: and float32 as well -- instantiations
    that take the element type at run time)"""
    return ([(f16(x), None), (bf16_bits(x), "bfloat16")] if h16 else [(x, None)]) + ([(x, None)] if h16 and f32 else [])


def ragged(T, uni):
    return None if uni else np.array([T, max(T - 3, 0), 0], np.int64)


# ---- the beam searches: wave, lane, generic --------------------------------------------------------------------------
# Set by tests/test_instantiation_ledger_emu.py: a callable that returns the names launched since it was last called (the
# emulator's launch log, read and reset).  With it, EVERY call of a beam row -- each T, each input form, each push of a
# session -- is held to "launched exactly the row's instantiation", not only the row as a whole.
PROBE = None


def _begin_call():
    if PROBE is not None:
        PROBE()


def _end_call(expect, what):
    if PROBE is not None and expect is not None:
        same = {n for n in PROBE() if parse(n)[0] == parse(expect)[0]}
        assert same == {expect}, "%s: the call launched %s, not %s" % (what, sorted(same), expect)


def _check_single(r, x, lengths, want_of, what):
    r = r.cpu()
    for i in range(x.shape[0]):
        Ti = x.shape[1] if lengths is None else int(lengths[i])
        SC.check_slot(r, i, want_of(i, Ti), "%s read %d" % (what, i))


def _check_nbest(r, x, lengths, hyps_of, amb_of, beam, what):
    r = r.cpu()
    lens = [x.shape[1]] * x.shape[0] if lengths is None else [int(v) for v in lengths]
    NC.check(r, [hyps_of(i, lens[i]) for i in range(x.shape[0])], beam, x.shape[0])
    if amb_of is not None:
        for i in range(x.shape[0]):
            if int(r.status[i]) == 0:
                got = tuple(int(v) for v in np.asarray(r.ambiguous[i]))
                assert got == amb_of(i, lens[i]), (what, i, got, amb_of(i, lens[i]))


def _session(fcd, make, x, T, lengths, forms, want_of, what, expect):
    """two pushes (one where T == 1), ragged in the second; each slot's result after every push against the oracle"""
    cut = (T + 1) // 2
    lens = np.full(B, T, np.int64) if lengths is None else lengths
    for xin, dt in forms:
        with make() as s:
            done = np.zeros(B, np.int64)
            for a, b in ((0, cut), (cut, T)):
                if b <= a:
                    continue
                take = np.clip(lens - a, 0, b - a)
                _begin_call()
                r = s.push(np.ascontiguousarray(xin[:, a:b]), None if lengths is None else take, result=True, input_dtype=dt).cpu()
                _end_call(expect, "%s rows %d..%d %s" % (what, a, b, xin.dtype))
                done += take
                for i in range(B):
                    SC.check_slot(r, i, want_of(i, int(done[i])), "%s rows %d..%d slot %d" % (what, a, b, i))


def crf_beam_host(fcd, x, init, beam, thr, lengths, kernel, count_ambiguous, input_dtype):
    """fcd_crf_beam_search_host_k with the batch's element type stated: api.crf_beam_search_batch_raw, which takes no
    input_dtype, restated on the C ABI so that bfloat16 bits reach the one-shot CRF instantiations too"""
    import ctypes as C

    from fast_ctc_decode_amd import _native as nat
    from fast_ctc_decode_amd import api
    x = np.ascontiguousarray(x)
    init = np.ascontiguousarray(init, np.float32)
    Bn, T = x.shape[:2]
    h = nat.default_handle()
    out = api._HostOut(Bn, T, want_amb=count_ambiguous)
    l = api._np_lengths(lengths, Bn)
    b = api._host_batch(x, True, l, input_dtype)
    h.check(h.lib.fcd_crf_beam_search_host_k(h.ptr, C.byref(b), init.ctypes.data, init.shape[1], init.shape[1], int(beam),
                                             float(thr), int(kernel), C.byref(out.res)))
    return api.BatchResult(out.labels, out.path, out.out_len, out.status, ambiguous=out.ambiguous)


def _memo(f):
    seen = {}

    def g(i, Ti):
        if (i, Ti) not in seen:
            seen[(i, Ti)] = f(i, Ti)
        return seen[(i, Ti)]
    return g


def beam_case(fcd, kernel, beam, N, S, amb, uni, h16, pdq, nb, ses, key, can_tie=True, expect=None, any_dtype=False):
    """one beam-search call per T and input form of the row: plain (S == 0) or CRF with S states.  h16: the row is selected
    by 16-bit input (binary16 AND bfloat16 bits); any_dtype: the instantiation takes the element type at run time, whatever
    selected it (n-best, the lane and generic kernels): float32, binary16 and bfloat16.  expect: the row's name, for PROBE"""
    order = "pdq178" if (pdq or not can_tie) else "stable"
    crf = S != 0
    with tie_order(fcd, order):
        for T in ts_of(key):
            lengths = ragged(T, uni)
            seed = 7 + T + 13 * N + S
            what = "%s T %d" % (key, T)
            if crf:
                x, init = crf_reads(S, T, seed, N)
                # (a slot without rows: OK and empty, as session_cases.run_crf asserts before the first push)
                want_of = _memo(lambda i, Ti: SC.want_crf(x[i, :Ti], init[i], beam, 0.0) if Ti else (SC.OK, [], [], (0, 0)))
                hyps_of = _memo(lambda i, Ti: NR.crf_beam_search(x[i, :Ti], init[i], beam, 0.0, stable=(order == "stable")))
            else:
                x = plain_reads(N, T, seed)
                want_of = _memo(lambda i, Ti: SC.want_plain(x[i, :Ti], beam, 0.0, True))
                hyps_of = _memo(lambda i, Ti: NR.beam_search(x[i, :Ti], beam, 0.0, True, stable=(order == "stable")))
            amb_of = (lambda i, Ti: tuple(int(v) for v in want_of(i, Ti)[3])) if amb else None
            forms = inputs_of(x, True, f32=True) if any_dtype else inputs_of(x, h16)
            if ses:
                if crf:
                    make = lambda: fcd.CrfBeamSearchSession(B, S, N, init, T, beam, 0.0, count_ambiguous=amb, kernel=kernel)
                else:
                    make = lambda: fcd.BeamSearchSession(B, N, T, beam, 0.0, True, count_ambiguous=amb, kernel=kernel)
                _session(fcd, make, x, T, lengths, forms, want_of, what, expect)
                continue
            for xin, dt in forms:
                _begin_call()
                if nb and crf:
                    r = fcd.crf_beam_search_nbest_batch_raw(xin, init, beam, beam, 0.0, lengths=lengths, kernel=kernel,
                                                            count_ambiguous=amb, input_dtype=dt)
                elif nb:
                    r = fcd.beam_search_nbest_batch_raw(xin, beam, beam, 0.0, True, lengths=lengths, kernel=kernel,
                                                        count_ambiguous=amb, input_dtype=dt)
                elif crf:
                    r = crf_beam_host(fcd, xin, init, beam, 0.0, lengths, kernel, amb, dt)
                else:
                    r = fcd.beam_search_batch_raw(xin, beam, 0.0, True, lengths=lengths, kernel=kernel, count_ambiguous=amb,
                                                  input_dtype=dt)
                _end_call(expect, "%s %s %s" % (what, xin.dtype, dt or ""))
                if nb:
                    _check_nbest(r, x, lengths, hyps_of, amb_of, beam, what)
                else:
                    assert (r.ambiguous is not None) == amb
                    _check_single(r, x, lengths, want_of, what)


# beam_wave_kernel<N, GW, RPW, S, AMB, PROF, UNI, H16, PDQ, NB, SES>   (S: 0 plain, 4 the register FIFO, -1 the row gather)
WAVE_SHAPES = ([(n, 5, 1, 0) for n in (3, 4, 5)] + [(n, 6, 2, 0) for n in (3, 4, 5)] + [(n, 8, 1, 0) for n in (3, 4, 5, 6, 7)] +
               [(5, g, r, s) for s in (4, -1) for g, r in ((5, 1), (6, 2), (8, 1))])
# (AMB, UNI, H16, NB, SES) of launch_tp (beam_wave.hip:611) and ses_tp (beam_wave_session.hip:12)
WAVE_VARIANTS = [(True, False, True, True, False), (False, False, True, True, False),      # n-best
                 (True, False, True, False, False), (False, False, True, False, False),    # 16-bit posteriors
                 (True, False, False, False, False), (False, True, False, False, False), (False, False, False, False, False),
                 (True, False, True, False, True), (False, False, True, False, True),      # sessions
                 (True, False, False, False, True), (False, False, False, False, True)]
WAVE_BEAM = {(6, 2): 5, (8, 1): 8, (5, 1): 12}


def wave_can_tie(N, GW, RPW):
    return ((64 // RPW) // GW) * N > 20  # (launch_t, beam_wave.hip:651)


def wave_rows():
    for N, GW, RPW, S in WAVE_SHAPES:
        for pdq in ((False, True) if wave_can_tie(N, GW, RPW) else (False,)):
            for amb, uni, h16, nb, ses in WAVE_VARIANTS:
                yield (N, GW, RPW, S, amb, False, uni, h16, pdq, nb, ses)


def wave_case(fcd, args):
    N, GW, RPW, S, amb, prof, uni, h16, pdq, nb, ses = args
    assert not prof
    beam = WAVE_BEAM[(GW, RPW)]
    # groups of eight at N <= 5: the force-one-read-per-wave kernel id (beam 8 alone selects them as well)
    kernel = KERNEL_WAVE1 if (GW, RPW) == (8, 1) and N <= 5 else KERNEL_WAVE
    # (the n-best instantiations carry H16 = true whatever the input: float32, binary16 and bfloat16 all reach them)
    beam_case(fcd, kernel, beam, N, {0: 0, 4: 4, -1: 8}[S], amb, uni, h16, pdq, nb, ses, ("wave",) + args,
              can_tie=wave_can_tie(N, GW, RPW), expect=spell("beam_wave_kernel", args), any_dtype=nb)


# beam_lane_kernel<N, RPW, AMB, CRF, PDQ, NB>: launch_beam_lane, launch_na, launch_nap (beam_lane.hip:1085-1224)
LANE_BEAM = {2: 13, 1: 40}  # (beam_lane_reads_per_wave: two reads per wavefront up to beam 32)


def lane_rows():
    for N, crf in [(n, False) for n in range(2, 9)] + [(5, True)]:
        for rpw in (1, 2):
            for amb in (False, True):
                for pdq in (False, True):
                    for nb in (False, True):
                        yield (N, rpw, amb, crf, pdq, nb)


def lane_case(fcd, args):
    N, rpw, amb, crf, pdq, nb = args
    # (the lane kernels take the element type at run time: every row feeds float32, binary16 and bfloat16)
    beam_case(fcd, KERNEL_LANE, LANE_BEAM[rpw], N, 4 if crf else 0, amb, False, False, pdq, nb, False, ("lane",) + args,
              expect=spell("beam_lane_kernel", args), any_dtype=True)


# beam_generic_kernel<NB, SES>: launch_beam_generic (beam_generic.hip:703-708); plain and CRF reads share an instantiation
def generic_rows():
    return [(False, False), (True, False), (False, True)]


def generic_case(fcd, args):
    nb, ses = args
    for crf in (False, True):
        beam_case(fcd, KERNEL_GENERIC, 5, 4 if crf else 9, 3 if crf else 0, True, False, False, True, nb, ses,
                  ("generic", nb, ses, crf), expect=spell("beam_generic_kernel", args), any_dtype=True)


# ---- the greedy searches (viterbi.hip) -----------------------------------------------------------------------------------
def _greedy_values(rng, shape):
    """reads in turn: quantised k / 4 with zeros (argmax ties: the first maximum wins) and k / 256; exact in 16 bits"""
    x = (rng.integers(0, 5, size=shape) / 4.0).astype(np.float32)
    x[1::2] = rng.integers(1, 257, size=x[1::2].shape) / 256.0
    return x


def _as_dtype(x, dt):
    """(array, input_dtype) of dtype code 0 float32, 1 binary16, 2 bfloat16 bits"""
    return [(x, None), (f16(x), None), (bf16_bits(x), "bfloat16")][dt]


def _viterbi_check(fcd, view, up, lengths, input_dtype):
    for collapse, qual in ((True, True), (False, False)):
        r = fcd.viterbi_search_batch_raw(view, collapse, lengths=lengths, qual=qual, input_dtype=input_dtype)
        for i in range(up.shape[0]):
            Ti = up.shape[1] if lengths is None else int(lengths[i])
            n = int(r.out_len[i])
            if Ti == 0:
                assert n == 0, i
                continue
            labels, path, quals = oracle.viterbi_search_raw(np.ascontiguousarray(up[i, :Ti]), collapse)
            assert n == len(labels), (i, collapse)
            np.testing.assert_array_equal(r.labels[i, :n], labels)
            np.testing.assert_array_equal(r.path[i, :n], path)
            if qual:
                got = [oracle.lib.fcdo_phred(float(q), 1.0, 0.0) for q in r.qual[i, :n]]
                assert [ord(c) for c in got] == list(quals), i


# viterbi_stream_kernel<N, dtype>: launch_viterbi's stream_ok (viterbi.hip:803, :843): C-contiguous rows, reads on 16-byte
# boundaries (T * N a multiple of 8 elements), N in 2 .. 8.  T = 264: past the 256-row tile; five reads: two workgroups
def viterbi_stream_case(fcd, args):
    N, dt = args
    T = 264
    x = _greedy_values(np.random.default_rng(40 + N), (5, T, N))
    xin, idt = _as_dtype(x, dt)
    _viterbi_check(fcd, xin, x, np.array([T, T - 3, 0, 1, 257], np.int64), idt)
    _viterbi_check(fcd, xin[:, :72], x[:, :72], None, idt)


# viterbi_tm_kernel<N, dtype>: tm_ok (viterbi.hip:807): (T, B, N) storage seen as a batch, at least 8 reads, rows of the
# storage on 16-byte boundaries.  16 reads stored, 11 handed over: one group of eight, three on viterbi_kernel
def viterbi_tm_case(fcd, args):
    N, dt = args
    T = 72
    x = _greedy_values(np.random.default_rng(50 + N), (16, T, N))
    xin, idt = _as_dtype(x, dt)
    view = np.ascontiguousarray(xin.transpose(1, 0, 2)).transpose(1, 0, 2)[:11]
    lengths = np.array([T, T - 3, 0, 1, T, 65, 64, 7, T, 2, T - 1], np.int64)
    _viterbi_check(fcd, view, x[:11], lengths, idt)
    _viterbi_check(fcd, view, x[:11], None, idt)


def viterbi_case(fcd, args):  # viterbi_kernel: N outside 2 .. 8 (viterbi.hip:860)
    x = _greedy_values(np.random.default_rng(60), (3, 65, 9))
    _viterbi_check(fcd, x, x, np.array([65, 62, 0], np.int64), None)


def _crf_greedy_check(fcd, view, init, lengths):
    Bn, T, S, N = view.shape
    alpha = "NACGTUV"[:N]
    r = fcd.crf_greedy_search_batch_raw(view, init, lengths, qual=True)
    for i in range(Bn):
        Ti = T if lengths is None else int(lengths[i])
        if Ti == 0:
            assert int(r.out_len[i]) == 0, i
            continue
        xi = np.ascontiguousarray(view[i, :Ti])
        try:
            seq, path = oracle.crf_greedy_search(xi, init[i], alpha, False)
        except RuntimeError:
            assert int(r.status[i]) == fcd.api.nat.ST_BAD_STATE, i
            continue
        assert int(r.status[i]) == 0, i
        n = int(r.out_len[i])
        assert "".join(alpha[l] for l in r.labels[i, :n]) == seq and r.path[i, :n].tolist() == path, i
        qs = oracle.crf_greedy_search(xi, init[i], alpha, True)[0][n:]
        assert "".join(oracle.phred(float(q)) for q in r.qual[i, :n]) == qs, i


# crf_greedy_stream_kernel<S, TM>: launch_crf_greedy (viterbi.hip:870-908): float32, S in 1 .. 8, S * N <= 32; TM: (T, B, S, N)
# storage with at least four reads.  N = 4 fits every S; TM: eight reads stored, six handed over (two on crf_greedy_kernel)
def crf_greedy_stream_case(fcd, args):
    S, tm = args
    T, N = 66, 4
    rng = np.random.default_rng(70 + S)
    x = _greedy_values(rng, (8, T, S, N))
    init = rng.random((8, S), dtype=np.float32)
    if tm:
        view = np.ascontiguousarray(x.transpose(1, 0, 2, 3)).transpose(1, 0, 2, 3)[:6]
        _crf_greedy_check(fcd, view, init[:6], np.array([T, T - 3, 0, 1, T, 65], np.int64))
        _crf_greedy_check(fcd, view, init[:6], None)
    else:
        _crf_greedy_check(fcd, x[:5], init[:5], np.array([T, T - 3, 0, 1, T], np.int64))
        _crf_greedy_check(fcd, x[:5], init[:5], None)


def crf_greedy_case(fcd, args):  # crf_greedy_kernel: S above 8 (viterbi.hip:922)
    rng = np.random.default_rng(80)
    x = _greedy_values(rng, (3, 65, 9, 4))
    _crf_greedy_check(fcd, x, rng.random((3, 9), dtype=np.float32), np.array([65, 62, 0], np.int64))


# ---- the CRF walks over all labellings: one kernel each, whose code forms are chosen at run time from S and N.  One entry
# of the walk's own case table per form, the smallest that reaches it, checked by that table's run_case ------------------------
def crf_viterbi_case(fcd, args):
    """crf_viterbi_kernel (crf_viterbi.hip:117, :170, :188): a lane per element (S N <= 64), a lane per state (S <= 64),
    several states per lane with two passes per row; T = 65 crosses the 64-emission flush of the walk back"""
    import crf_viterbi_cases as VC
    for S, N, T in ((4, 5, 65), (64, 5, 65), (256, 3, 65)):
        case, = [c for c in VC.CASES if c[1:4] == (S, N, T)]
        VC.run_case(fcd, VC.build_case(case))


def crf_transitions_case(fcd, args):
    """crf_transitions_kernel (crf_transitions.hip:64, :104): a lane per element, a lane per state with one chunk of 64
    states, and with many"""
    import crf_transitions_cases as TC
    for name in ("s4_n5_t7_dest_f16in", "s64_n5_t7_bf16_padded", "s256_n5_t65_dest_tm"):
        case, = [c for c in TC.CASES if c["name"] == name]
        TC.run_case(fcd, case)


def crf_marginals_case(fcd, args):
    """crf_marginals_kernel (crf_transitions.hip:255, :291): the forward pass's forms, behind the same three of the walk"""
    import crf_marginals_cases as MC
    for name in ("s4_n5_t7_dest_f16", "s64_n5_t2_bf16_padded", "s256_n5_t65_dest_tm"):
        MC.run_case(fcd, MC.by_name(name))


# ---- the lattice walks: the run_case functions of their case files, at the T that selects the instantiation ----------
# CTC (ctc_score.hip:220-238, ctc_align.hip:369-428, ctc_posterior.hip:583-664): an exact window holds 2 T + 1 states (the
# labellings' stride is T), and K = 2 / 4 / 6 / 8 states per lane hold 126 / 254 / 382 / 510; more goes to LDS
CTC_T = {2: 30, 4: 63, 6: 127, 8: 191, 0: 255}  # (the smallest T of each K but the first; 0: the LDS kernels)


def _ctc_case(fcd, K, N, tag):
    import ctc_score_cases as CS
    T = CTC_T[K]
    # (name, N, T, B, n_hyp, dtype, time_major, collapse, ragged, bands): two reads, the second one shorter
    return CS.build_case(fcd, ("ledger-%s-k%d-n%d" % (tag, K, N), N, T, 2, 1, "f32", False, True, True, (0,)))


def score_reg_case(fcd, args):
    import ctc_score_cases as CS
    CS.run_case(fcd, _ctc_case(fcd, args[0], 5, "score"))


def score_lds_case(fcd, args):
    import ctc_score_cases as CS
    CS.run_case(fcd, _ctc_case(fcd, 0, 5, "score"))


def align_reg_case(fcd, args):
    import ctc_align_cases as CA
    CA.run_case(fcd, _ctc_case(fcd, args[0], 5, "align"))


def align_lds_case(fcd, args):
    import ctc_align_cases as CA
    CA.run_case(fcd, _ctc_case(fcd, 0, 5, "align"))


def post_fwd_case(fcd, args):
    import ctc_posterior_cases as CP
    CP.run_case(fcd, _ctc_case(fcd, args[0], 3, "post"))


def post_back_case(fcd, args):  # <K, NC>: NC = 4 up to four labels, 8 above (ctc_posterior.hip:628)
    import ctc_posterior_cases as CP
    CP.run_case(fcd, _ctc_case(fcd, args[0], 3 if args[1] == 4 else 6, "post"))


def edit_back_case(fcd, args):  # (ctc_posterior.hip:625)
    import ctc_edits_cases as CE
    CE.run_case(fcd, _ctc_case(fcd, args[0], 3 if args[1] == 4 else 6, "edits"))


# CRF (crf_lattice.h:358, crf_lattice.hip:108): an exact window holds T + 1 states; K = 1 / 2 / 4 / 8 hold 64 / 128 / 256 / 512
CRF_T = {1: 40, 2: 64, 4: 128, 8: 256}


def _crf_case(S, N, T, tag):
    import crf_lattice_cases as CC
    # (name, S, N, T, B, n_hyp, dtype, layout, bands, fill)
    return CC.build_case(("ledger_%s_s%dn%d_t%d" % (tag, S, N, T), S, N, T, 2, 1, "f32", "read", (0,), 0.7))


def crf_lattice_case(fcd, args):
    """<MAX, K>: crf_align (MAX) or crf_score alone, checked as crf_lattice_cases.run_case checks each"""
    import crf_lattice_cases as CC
    import crf_lattice_reference as R
    c = _crf_case(4, 5, CRF_T[args[1]], "lat")
    call = (c["xin"], c["init"], c["labels"], c["out_len"], c["lengths"], None, 0, c["n_valid"])
    if args[0]:
        got = fcd.crf_align_batch_raw(*call).cpu()
        CC.check(got, None, c["x32"], c["init"], c["lengths"], c["labels"], c["paths"], c["out_len"], c["n_valid"], 0)
        return
    score = fcd.crf_score_batch_raw(*call)
    for b in range(c["B"]):
        Tr = int(c["lengths"][b])
        want = R.crf_score(c["x32"][b, :Tr], c["init"][b], c["labels"][b, 0, :int(c["out_len"][b, 0])], 0, None)
        assert math.isfinite(want) and abs(score[b, 0] - want) <= CC.tolerance(Tr), (b, score[b, 0], want)


# crfp_back_kernel<K, MM, NB> (crf_posterior.hip:344-351, :386-393, :429-435): the tier follows from the chain m (S = nb^m)
# and the labels nb = N - 1; tiers of MM 1 / 2 / 4 hold K = 1, 2, 4 (, 8) as crf_lattice, those of MM 3 / 6 hold 1, 2, 3
# states per lane at up to 64 / 128 / 192 states
CRFP_TIER = {(1, 8): (8, 9), (2, 4): (16, 5), (4, 2): (8, 3), (3, 8): (64, 5), (6, 4): (1024, 5)}  # (MM, NB) -> (S, N)


def crfp_rows():
    return ([(k, 1, 8) for k in (1, 2, 4)] + [(k, 2, 4) for k in (1, 2, 4, 8)] + [(k, 4, 2) for k in (1, 2, 4, 8)] +
            [(k, 3, 8) for k in (1, 2, 3)] + [(k, 6, 4) for k in (1, 2, 3)])


def crfp_back_case(fcd, args):
    import crf_posterior_cases as CRP
    K, MM, NB = args
    S, N = CRFP_TIER[(MM, NB)]
    T = 128 if K == 3 else CRF_T[K]
    CRP.run_case(fcd, _crf_case(S, N, T, "post"))


def crfp_fwd_case(fcd, args):
    K = args[0]
    crfp_back_case(fcd, (K, 3, 8) if K == 3 else (K, 2, 4))


# ---- the duplex searches ------------------------------------------------------------------------------------------------
def _duplex_check(fcd, beam, mode, width=16, T=(40, 44), Bn=3):
    import platform

    import test_gpu_duplex as D
    x1, x2 = D.pairs(900 + beam + 7 * mode, Bn, T[0], T[1])
    envs = np.stack([D.band(T[0], T[1], width)] * Bn)
    name = {0: D.LSE, 1: D.MAX, 2: "logsumexp_glibc235"}[mode]
    got = D.gpu_strings(fcd, x1, x2, "NACGT", envs, beam, 0.05, True, name)
    if mode == 2:  # the host libm's arithmetic: the oracle's own where the host links glibc 2.35 (as test_gpu_duplex.py)
        want = D.oracle_strings(x1, x2, "NACGT", envs, beam, 0.05, True, D.LSE)
        if platform.libc_ver() != ("glibc", "2.35"):
            # another libm: the oracle is no exact reference for this mode (test_gpu_duplex holds the default flavour to
            # 90 % of the pairs against it).  Of these Bn = 3 pairs that allows no miss; were Bn to grow, one in ten
            assert sum(g != w for g, w in zip(got, want)) <= len(want) // 10, (got, want)
            return
    else:
        want = D.oracle_strings(x1, x2, "NACGT", envs, beam, 0.05, True, (D.LSE if mode == 0 else D.MAX) | D.CR)
    assert got == want


# duplex_slots_kernel<MODE, PROF>: duplex_dev takes it wherever beam_size * N <= 64 fits (capi.hip:1206-1215)
def duplex_slots_case(fcd, args):
    assert not args[1]
    _duplex_check(fcd, 5, args[0])


# duplex_kernel<MODE, PIN>: beam_size * N above the 64 slots (beam 16); PIN = the staged LOGSUMEXP form (duplex.hip:1599);
# a band of +-300 rows does not fit the LDS tile: unstaged, <0, false> (test_gpu_duplex.test_duplex_wide_band_unstaged_path)
def duplex_case(fcd, args):
    mode, pin = args
    if mode == 0 and not pin:
        _duplex_check(fcd, 16, 0, width=300, T=(330, 330), Bn=2)
    else:
        _duplex_check(fcd, 16, mode)


def ln_convert_case(fcd, args):  # ln_convert_kernel and env_width_kernel run ahead of every duplex search (capi.hip:1188-1193)
    _duplex_check(fcd, 5, 1)


def envelope_case(fcd, args):  # envelope_kernel and max_u32_kernel: fcd_duplex_envelope_* (capi.hip:1400, :1429)
    import test_gpu_envelope as E
    for seed in (0, 1, 3):
        E.test_envelope_equals_model(fcd, seed)


# ---- the rest ---------------------------------------------------------------------------------------------------------------
def session_restart_case(fcd, args):  # fcd_beam_session_restart (capi.hip:2390)
    SC.run_restart(fcd, 5, 5, KERNEL_WAVE)
    SC.run_crf_restart(fcd, 5, 4, 5, KERNEL_WAVE)


def slab_pool_case(fcd, args):
    """slab_pool_init_kernel: a workspace limit below the worst-case arena of a wide-beam job sends it down the two-pass
    path, whose slabs a device-side pool hands out (capi.hip:454, :519)"""
    from fast_ctc_decode_amd import _native as nat
    h = nat.default_handle()
    x = plain_reads(5, 65, 3)
    lengths = ragged(65, False)
    h.set_workspace_limit(256 << 10)
    try:
        for _ in range(2):
            r = fcd.beam_search_batch_raw(x, 20, 0.0, True, lengths=lengths, kernel=KERNEL_LANE)
            _check_single(r, x, lengths, lambda i, Ti: SC.want_plain(x[i, :Ti], 20, 0.0, True), "two-pass")
    finally:
        h.set_workspace_limit(0)


def _tensor(a, device):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if device is None else t.to(device)


def pack_case(fcd, args, device=None):
    """result_offsets_kernel, pack_kernel, unpack_kernel, gathered_offsets_kernel, gathered_unpack_kernel (pack.hip) take
    device pointers: torch tensors on `device` (the emulator's device memory is the host's).  The packed bytes against
    dist.pack_result, the numpy packer; both unpacks give the results back."""
    import torch

    from fast_ctc_decode_amd import _native as nat
    h = nat.default_handle()
    if device is not None:
        h.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        _pack_body(h, device)
    finally:
        if device is not None:
            h.synchronize()
            h.reset_stream()


def _pack_body(h, device):
    import ctypes as C

    from fast_ctc_decode_amd import _native as nat
    from fast_ctc_decode_amd import dist as fdist
    from fast_ctc_decode_amd.api import BatchResult
    import torch
    W = 37
    rng = np.random.default_rng(5)
    counts = [5, 0, 130, 1]
    shards, packed, totals = [], [], []
    for Bn in counts:
        out_len = rng.integers(0, W + 1, size=Bn).astype(np.int32)
        labels = np.zeros((Bn, W), np.uint8)
        path = np.zeros((Bn, W), np.int32)
        for i in range(Bn):
            labels[i, :out_len[i]] = rng.integers(1, 5, size=out_len[i])
            path[i, :out_len[i]] = np.sort(rng.integers(0, 60000, size=out_len[i]))
        status = rng.integers(0, 3, size=Bn).astype(np.int32)
        out_len[status != 0] = 0
        r = BatchResult(torch.from_numpy(labels), torch.from_numpy(path), torch.from_numpy(out_len), torch.from_numpy(status))
        shards.append(r)
        offs, total = fdist.result_total(r)
        totals.append(total)
    nbytes = max(fdist.packed_nbytes(max(counts), t, W) for t in totals)

    def same(r, got_labels, got_path, got_len, got_status):
        assert np.array_equal(r.out_len.numpy(), got_len) and np.array_equal(r.status.numpy(), got_status)
        for i in range(len(got_len)):
            n = int(got_len[i])
            assert np.array_equal(r.labels.numpy()[i, :n], got_labels[i, :n]) and np.array_equal(r.path.numpy()[i, :n], got_path[i, :n])

    full = np.zeros(nbytes * len(counts), np.uint8)
    for k, (r, Bn) in enumerate(zip(shards, counts)):
        if not Bn:
            continue
        offs_host, total = fdist.result_total(r)
        want = fdist.pack_result(r, offs_host, nbytes).numpy()
        d = [_tensor(a.numpy(), device) for a in (r.labels, r.path, r.out_len, r.status)]
        offs = _tensor(np.zeros(Bn + 1, np.int64), device)
        h.check(h.lib.fcd_result_offsets_dev(h.ptr, d[2].data_ptr(), Bn, W, offs.data_ptr()))
        assert np.array_equal(offs.cpu().numpy(), offs_host.numpy())
        buf = _tensor(np.zeros(nbytes, np.uint8), device)
        res = nat.Result(d[0].data_ptr(), d[1].data_ptr(), None, d[2].data_ptr(), d[3].data_ptr(), W)
        h.check(h.lib.fcd_pack_results_dev(h.ptr, C.byref(res), Bn, 2, offs.data_ptr(), buf.data_ptr()))
        got = buf.cpu().numpy()
        lab_end, path_at = 16 + 8 * Bn + total, 16 + 8 * Bn + ((total + 3) & ~3)  # (padding bytes are unspecified)
        assert np.array_equal(got[:lab_end], want[:lab_end])
        assert np.array_equal(got[path_at:path_at + 2 * total], want[path_at:path_at + 2 * total])
        full[k * nbytes:(k + 1) * nbytes] = want
        back = [_tensor(np.zeros(sh, dt), device) for sh, dt in (((Bn, W), np.uint8), ((Bn, W), np.int32), (Bn, np.int32), (Bn, np.int32))]
        res2 = nat.Result(back[0].data_ptr(), back[1].data_ptr(), None, back[2].data_ptr(), back[3].data_ptr(), W)
        work = _tensor(np.zeros(Bn + 1, np.int64), device)
        h.check(h.lib.fcd_unpack_results_dev(h.ptr, buf.data_ptr(), Bn, work.data_ptr(), C.byref(res2)))
        h.synchronize()
        same(r, *[b.cpu().numpy() for b in back])
    n_total = sum(counts)
    first = _tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), device)
    out = [_tensor(np.zeros(sh, dt), device) for sh, dt in (((n_total, W), np.uint8), ((n_total, W), np.int32), (n_total, np.int32), (n_total, np.int32))]
    work = _tensor(np.zeros(n_total + len(counts) + 1, np.int64), device)
    bad = _tensor(np.zeros(1, np.int32), device)
    res = nat.Result(out[0].data_ptr(), out[1].data_ptr(), None, out[2].data_ptr(), out[3].data_ptr(), W)
    fullt = _tensor(full, device)
    h.check(h.lib.fcd_unpack_gathered_dev(h.ptr, fullt.data_ptr(), nbytes, len(counts), first.data_ptr(), n_total,
                                          work.data_ptr(), C.byref(res), bad.data_ptr()))
    h.synchronize()
    assert int(bad.cpu()[0]) == 0
    o = [t.cpu().numpy() for t in out]
    row = 0
    for r, Bn in zip(shards, counts):
        same(r, *[a[row:row + Bn] for a in o])
        row += Bn


NEEDS_DEVICE_POINTERS = {"result_offsets_kernel", "pack_kernel", "unpack_kernel", "gathered_offsets_kernel", "gathered_unpack_kernel"}

_one = lambda: [()]
FAMILIES = {
    "viterbi_stream_kernel": (lambda: [(n, dt) for n in range(2, 9) for dt in (0, 1, 2)], viterbi_stream_case),
    "viterbi_tm_kernel": (lambda: [(n, dt) for n in range(2, 9) for dt in (0, 1, 2)], viterbi_tm_case),
    "viterbi_kernel": (_one, viterbi_case),
    "crf_greedy_stream_kernel": (lambda: [(s, tm) for s in range(1, 9) for tm in (False, True)], crf_greedy_stream_case),
    "crf_greedy_kernel": (_one, crf_greedy_case),
    "crf_viterbi_kernel": (_one, crf_viterbi_case),
    "crf_transitions_kernel": (_one, crf_transitions_case),
    "crf_marginals_kernel": (_one, crf_marginals_case),
    "score_reg_kernel": (lambda: [(k,) for k in (2, 4, 6, 8)], score_reg_case),
    "score_lds_kernel": (_one, score_lds_case),
    "align_reg_kernel": (lambda: [(k,) for k in (2, 4, 6, 8)], align_reg_case),
    "align_lds_kernel": (_one, align_lds_case),
    "post_fwd_kernel": (lambda: [(k,) for k in (2, 4, 6, 8)], post_fwd_case),
    "post_back_kernel": (lambda: [(k, nc) for k in (2, 4, 6, 8) for nc in (4, 8)], post_back_case),
    "edit_back_kernel": (lambda: [(k, nc) for k in (2, 4, 6, 8) for nc in (4, 8)], edit_back_case),
    "crf_lattice_kernel": (lambda: [(a, k) for a in (False, True) for k in (1, 2, 4, 8)], crf_lattice_case),
    "crfp_fwd_kernel": (lambda: [(k,) for k in (1, 2, 3, 4, 8)], crfp_fwd_case),
    "crfp_back_kernel": (crfp_rows, crfp_back_case),
    "duplex_slots_kernel": (lambda: [(m, False) for m in (0, 1, 2)], duplex_slots_case),
    "duplex_kernel": (lambda: [(0, False), (0, True), (1, False), (2, False)], duplex_case),
    "ln_convert_kernel": (_one, ln_convert_case),
    "env_width_kernel": (_one, ln_convert_case),
    "envelope_kernel": (_one, envelope_case),
    "max_u32_kernel": (_one, envelope_case),
    "session_restart_kernel": (_one, session_restart_case),
    "slab_pool_init_kernel": (_one, slab_pool_case),
    "result_offsets_kernel": (_one, pack_case),
    "pack_kernel": (_one, pack_case),
    "unpack_kernel": (_one, pack_case),
    "gathered_offsets_kernel": (_one, pack_case),
    "gathered_unpack_kernel": (_one, pack_case),

    "beam_wave_kernel": (wave_rows, wave_case),
    "beam_lane_kernel": (lane_rows, lane_case),
    "beam_generic_kernel": (generic_rows, generic_case),
}

# Kernels that no entry point of include/fcd.h can reach in a default build: (name, the dispatch line that says so)
EXEMPT = [
    ("beam_wave_kernel<5,6,2,0,false,true,false,false,false,false,false>",
     "beam_wave.hip:635 `p.a.prof && ...`: BeamArgs.prof is set by fcd_beam_search_profile_dev alone (capi.hip:1052, fcd_debug.h)"),
    ("beam_wave_kernel<5,6,2,0,false,true,false,false,true,false,false>",
     "beam_wave.hip:635 `p.a.prof && ...`: BeamArgs.prof is set by fcd_beam_search_profile_dev alone (capi.hip:1052, fcd_debug.h)"),
] + [
    ("duplex_slots_kernel<%d,true>" % m,
     "duplex_slots.hip:1501 `if (a.prof)`: DuplexArgs.prof is fcd_handle::duplex_prof (capi.hip:1256), set by "
     "fcd_debug_set_duplex_profile alone (capi.hip:958, fcd_debug.h)") for m in (0, 1, 2)
] + [
    ("logspace_probe_kernel", "duplex.hip:1564 launch_logspace_probe: fcd_logspace_probe_dev alone (capi.hip:1470, fcd_debug.h)"),
    ("glibc235_apply_kernel", "duplex.hip:1556 launch_glibc235_apply: fcd_debug_glibc235_dev alone (capi.hip:1479, fcd_debug.h)"),
    ("logadd_sweep_kernel", "duplex.hip:1570 launch_logadd_sweep: fcd_logadd_sweep_dev alone (capi.hip:1489, fcd_debug.h)"),
    ("logadd_chain_kernel<0>", "duplex.hip:1578 launch_logadd_chain: fcd_logadd_latency_probe_dev alone (capi.hip:1498, fcd_debug.h)"),
    ("logadd_chain_kernel<1>", "duplex.hip:1576 launch_logadd_chain: fcd_logadd_latency_probe_dev alone (capi.hip:1498, fcd_debug.h)"),
    ("pdq178_probe_kernel", "tieorder.hip:85 launch_pdq178_probe: fcd_debug_pdq178_sort_dev alone (capi.hip:924, fcd_debug.h)"),
] + [
    ("pdq178_wave_probe_kernel<%d>" % n,
     "tieorder.hip:58-61 launch_pdq178_coop_probe: fcd_debug_pdq178_coop_sort_dev alone (capi.hip:935, fcd_debug.h)") for n in (1, 3, 5, 8)
]


def rows():
    """every (canonical name, family case function, template arguments) of the ledger"""
    out = []
    for template, (enum, case) in FAMILIES.items():
        for args in enum():
            out.append((spell(template, args), case, tuple(args)))
    return out


def run(fcd, name, device=None):
    """device: where the rows that take device pointers put their tensors (None: the emulator, whose device memory is the
    host's; "cuda" on the GPU)"""
    template, args = parse(name)
    if template in NEEDS_DEVICE_POINTERS:
        FAMILIES[template][1](fcd, args, device)
    else:
        FAMILIES[template][1](fcd, args)
