"""Host-side mirror of fast_ctc_decode's Python surface (/root/reference/src/lib.rs:142-628)
over the HIP C ABI (include/fcd.h).

Single-read functions keep the reference's names, argument order, defaults, validation order,
exception types and messages, so they are a drop-in.  The `*_batch` functions are additive:
they decode many reads per launch (numpy -> staged through the C ABI's *_host entry points;
torch tensors on an AMD GPU -> zero-copy through the *_dev entry points on the tensor's
current stream).  All searching happens on the GPU: there is no CPU fallback.
"""
import contextlib
import ctypes as C

import numpy as np

from . import _native as nat

__version__ = "0.3.7"  # the reference version this surface mirrors (Cargo.toml:3)

_cm = None


def _compiled():
    """The compiled host layer (csrc/pymodule.cpp, module `fast_ctc_decode`): the batch functions on HOST inputs
    are its batch functions -- one implementation of chunk streaming, string and path building."""
    global _cm
    if _cm is None:
        import importlib.util
        import os

        from . import build as _build
        nat.load()  # libfcd_hip.so (and torch's HIP runtime before it) first
        path = _build.pymodule_path()
        if not os.path.exists(path):
            _build.build_pymodule()
        spec = importlib.util.spec_from_file_location("fast_ctc_decode", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _cm = mod
    return _cm


# ---------------------------------------------------------------------------------------------
# argument conversion / validation, as the PyO3 wrappers do it
# ---------------------------------------------------------------------------------------------
def _seq_to_vec(alphabet):
    """src/lib.rs:143-146: PySequence -> tuple -> str() of every element."""
    try:
        return [str(x) for x in tuple(alphabet)]
    except TypeError:
        raise TypeError("alphabet must be a sequence")


def _as_f32(a, ndim, name):
    """PyO3 extracts &PyArrayN<f32>; anything else is a TypeError (no implicit casts)."""
    if not isinstance(a, np.ndarray):
        raise TypeError("argument '%s': expected numpy.ndarray, got %s" % (name, type(a).__name__))
    if a.dtype != np.float32 or a.ndim != ndim:
        raise TypeError("argument '%s': expected a %d-dimensional float32 array, got %d-dimensional %s"
                        % (name, ndim, a.ndim, a.dtype))
    return a


def _usize(v, name):
    """PyO3's extraction of a `usize` argument: it happens before the function body, i.e. before every check
    of src/lib.rs -- a negative int is an OverflowError, anything but an int a TypeError."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError("argument '%s': expected an integer" % name)
    if v < 0:
        raise OverflowError("can't convert negative int to unsigned")
    return int(v)


def _check_beam_args(n_alpha, inner, beam_size, thr):
    """src/lib.rs:331-349 -- the order of these checks is part of the behaviour."""
    _usize(beam_size, "beam_size")
    f32 = np.float32
    max_beam_cut = f32(1.0) / f32(n_alpha) if n_alpha else f32(np.inf)
    if n_alpha != inner:
        raise ValueError("alphabet size %d does not match probability matrix inner dimension %d"
                         % (n_alpha, inner))
    if beam_size == 0:
        raise ValueError("beam_size cannot be 0")
    if f32(thr) < f32(-0.0):
        raise ValueError("beam_cut_threshold must be at least 0.0")
    if f32(thr) >= max_beam_cut:
        raise ValueError("beam_cut_threshold cannot be more than %s" % max_beam_cut)


def _check_greedy_alphabet(n_alpha, inner):
    """src/lib.rs:190-195,227-232,264-269"""
    if n_alpha == 0:
        raise ValueError("Empty alphabet given")
    if n_alpha != inner:
        raise ValueError("alphabet size does not match probability matrix dimensions")


def _raise_status(st):
    if st != nat.ST_OK:
        raise RuntimeError(nat.status_string(st))  # src/lib.rs:363 map_err -> PyRuntimeError


def _estrides(a):
    return [s // a.itemsize for s in a.strides]


def _dense(a):
    """The C ABI's host staging copies one contiguous span; negative strides need a copy."""
    if any(s < 0 for s in a.strides):
        return np.ascontiguousarray(a)
    return a


# ---------------------------------------------------------------------------------------------
# low-level batched calls (host numpy buffers)
# ---------------------------------------------------------------------------------------------
class _HostOut:
    def __init__(self, B, T, want_path=True, want_qual=False, want_amb=False):
        w = max(int(T), 1)
        self.ambiguous = np.zeros((B, 2), np.uint32) if want_amb else None
        self.labels = np.zeros((B, w), np.uint8)
        self.path = np.zeros((B, w), np.uint32) if want_path else None
        self.qual = np.zeros((B, w), np.float32) if want_qual else None
        self.out_len = np.zeros(B, np.uint32)
        self.status = np.zeros(B, np.int32)
        self.res = nat.Result(
            self.labels.ctypes.data, self.path.ctypes.data if want_path else None,
            self.qual.ctypes.data if want_qual else None, self.out_len.ctypes.data,
            self.status.ctypes.data, w, self.ambiguous.ctypes.data if want_amb else None)


def _np_dtype_code(x, input_dtype=None):
    """float32 / float16 arrays carry their type; bfloat16 (numpy has none) travels as uint16 bit patterns with
    input_dtype="bfloat16"."""
    if input_dtype in ("bfloat16", nat.DTYPE_BF16):
        if x.dtype != np.uint16:
            raise TypeError("bfloat16 posteriors are passed as a uint16 array of bit patterns")
        return nat.DTYPE_BF16
    if x.dtype == np.float32:
        return nat.DTYPE_F32
    if x.dtype == np.float16:
        return nat.DTYPE_F16
    raise TypeError("expected a float32 or float16 array, got %s" % x.dtype)


def _host_batch(x, crf, lengths=None, input_dtype=None):
    """x: (B,T,N) or (B,T,S,N) numpy view (float32, float16, or uint16 bfloat16 bits) -> nat.Batch (the caller
    keeps x alive)."""
    st = _estrides(x)
    if crf:
        B, T, S, N = x.shape
        b = nat.Batch(x.ctypes.data, B, T, S, N, st[0], st[1], st[2], st[3], None)
    else:
        B, T, N = x.shape
        b = nat.Batch(x.ctypes.data, B, T, 1, N, st[0], st[1], 0, st[2], None)
    if lengths is not None:
        b.lengths = lengths.ctypes.data
    b.dtype = _np_dtype_code(x, input_dtype)
    return b


def _np_lengths(lengths, B):
    if lengths is None:
        return None
    l = np.ascontiguousarray(np.asarray(lengths), np.int64)
    if l.shape != (B,):
        raise ValueError("lengths must have shape (n_reads,)")
    return l


# ---------------------------------------------------------------------------------------------
# drop-in single-read API
# ---------------------------------------------------------------------------------------------
def _qual_chars(probs, qscale, qbias):
    lib = nat.load()
    return "".join(chr(lib.fcd_phred(float(p), float(qscale), float(qbias))) for p in probs)


_coalescer = None


def set_coalescing(max_batch=256, max_wait_us=0, device=0):
    """Route the per-read `viterbi_search` / `beam_search` / `crf_beam_search` / `crf_greedy_search` calls of ALL threads
    through one coalescer
    (include/fcd.h, csrc/coalesce.hip): calls that are in flight at the same time are decoded by one batched
    launch instead of one single-wavefront launch each.  Results do not change.  `max_batch=0` switches it
    off again.  Not in the reference (which has no batch notion); meant for callers that keep its per-read,
    many-threads calling pattern."""
    global _coalescer
    old, _coalescer = _coalescer, None
    if old is not None:
        old.close()
    if max_batch:
        _coalescer = nat.Coalescer(device, max_batch, max_wait_us)


def coalescing_stats():
    """{'calls', 'launches', 'largest_batch'} of the active coalescer, or None."""
    c = _coalescer
    return None if c is None else c.stats()


def viterbi_search(network_output, alphabet, qstring=False, qscale=1.0, qbias=0.0,
                   collapse_repeats=True):
    """Greedy (best-path) CTC decode.  Mirrors src/lib.rs:170-212 -> search.rs:320-383.

    Returns (str, list[int]): the sequence (with the quality string appended when `qstring`)
    and the row index of every emitted label."""
    x = _as_f32(network_output, 2, "network_output")
    alpha = _seq_to_vec(alphabet)
    _check_greedy_alphabet(len(alpha), x.shape[1])
    if x.shape[0] == 0:
        raise RuntimeError("network_output is empty (the reference asserts and aborts here)")
    x = _dense(x)
    out = _HostOut(1, x.shape[0], want_qual=bool(qstring))
    b = _host_batch(x[None], False)
    co = _coalescer
    if co is not None:
        with co:
            co.check(co.lib.fcd_coalescer_viterbi_search(co.ptr, C.byref(b), int(bool(collapse_repeats)),
                                                         C.byref(out.res)))
    else:
        h = nat.default_handle()
        h.check(h.lib.fcd_viterbi_search_host(h.ptr, C.byref(b), int(bool(collapse_repeats)),
                                              C.byref(out.res)))
    n = int(out.out_len[0])
    seq = "".join(alpha[l] for l in out.labels[0, :n])
    if qstring:
        seq += _qual_chars(out.qual[0, :n], qscale, qbias)
    return seq, [int(p) for p in out.path[0, :n]]


def beam_search(network_output, alphabet, beam_size=5, beam_cut_threshold=0.0,
                collapse_repeats=True, *, qstring=False, qscale=1.0, qbias=0.0):
    """CTC prefix beam search.  Mirrors src/lib.rs:318-365 -> search.rs:159-301.

    qstring=True (not in the reference, whose beam search has no qualities) appends a quality string to the sequence
    as viterbi_search does: each label's mean posterior over the rows the best alignment of the result gives it
    (ctc_align_batch_raw; the exact lattice where it fits, a band of 64 labels around the search's path otherwise)."""
    x = _as_f32(network_output, 2, "network_output")
    alpha = _seq_to_vec(alphabet)
    _check_beam_args(len(alpha), x.shape[1], beam_size, beam_cut_threshold)
    x = _dense(x)
    out = _HostOut(1, x.shape[0])
    b = _host_batch(x[None], False)
    co = _coalescer
    if co is not None:
        with co:
            co.check(co.lib.fcd_coalescer_beam_search(co.ptr, C.byref(b), int(beam_size), float(beam_cut_threshold),
                                                      int(bool(collapse_repeats)), C.byref(out.res)))
    else:
        h = nat.default_handle()
        h.check(h.lib.fcd_beam_search_host(h.ptr, C.byref(b), int(beam_size), float(beam_cut_threshold),
                                           int(bool(collapse_repeats)), nat.KERNEL_AUTO,
                                           C.byref(out.res)))
    _raise_status(int(out.status[0]))
    n = int(out.out_len[0])
    seq = "".join(alpha[l] for l in out.labels[0, :n])
    if qstring and n:
        try:
            al = ctc_align_batch_raw(x[None], out.labels, out.out_len, collapse_repeats)
        except nat.NativeError as e:
            if e.code != nat.E_UNSUPPORTED:  # (refused before anything is staged: the exact lattice does not fit)
                raise
            al = ctc_align_batch_raw(x[None], out.labels, out.out_len, collapse_repeats, paths=out.path, band=64)
        seq += al.qstrings(out.out_len, qscale, qbias)[0][0]
    return seq, [int(p) for p in out.path[0, :n]]


def crf_beam_search(network_output, init_state, alphabet, beam_size=5, beam_cut_threshold=0.0, *, qstring=False,
                    qscale=1.0, qbias=0.0):
    """Mirrors src/lib.rs:252-286 -> search.rs:38-157 (this wrapper validates only the alphabet).

    qstring=True (not in the reference, whose CRF beam search has no qualities) appends one phred character per label,
    as crf_greedy_search does: the posterior of each label's emission in the best alignment of the result
    (crf_align_batch_raw; the whole lattice where it fits, a band of 64 labels around the search's path otherwise)."""
    x = _as_f32(network_output, 3, "network_output")
    init = _as_f32(init_state, 1, "init_state")
    beam_size = _usize(beam_size, "beam_size")
    alpha = _seq_to_vec(alphabet)
    _check_greedy_alphabet(len(alpha), x.shape[2])
    if x.size == 0 or init.size == 0:
        raise RuntimeError("network_output/init_state is empty (the reference asserts and aborts here)")
    if beam_size < 1:
        raise RuntimeError(nat.status_string(nat.ST_RAN_OUT_OF_BEAM))  # truncate(0) -> empty beam
    x = _dense(x)
    init = np.ascontiguousarray(init)
    out = _HostOut(1, x.shape[0])
    b = _host_batch(x[None], True)
    co = _coalescer
    if co is not None:
        with co:
            co.check(co.lib.fcd_coalescer_crf_beam_search(co.ptr, C.byref(b), init.ctypes.data, init.shape[0],
                                                          int(beam_size), float(beam_cut_threshold), C.byref(out.res)))
    else:
        h = nat.default_handle()
        h.check(h.lib.fcd_crf_beam_search_host(h.ptr, C.byref(b), init.ctypes.data, init.shape[0],
                                               init.shape[0], int(beam_size), float(beam_cut_threshold),
                                               C.byref(out.res)))
    _raise_status(int(out.status[0]))
    n = int(out.out_len[0])
    labels = out.labels[0, :n]
    # search.rs:146-156: labels are appended leaf->root and the CHARACTERS reversed at the end
    seq = "".join(alpha[l] for l in labels[::-1])[::-1]
    if qstring and n:
        try:
            al = crf_align_batch_raw(x[None], init[None], out.labels, out.out_len)
        except nat.NativeError as e:
            if e.code != nat.E_UNSUPPORTED:  # (refused before anything is staged: the whole lattice does not fit)
                raise
            al = crf_align_batch_raw(x[None], init[None], out.labels, out.out_len, paths=out.path, band=64)
        seq += al.qstrings(out.out_len, qscale, qbias)[0][0]
    return seq, [int(p) for p in out.path[0, :n]]


def crf_greedy_search(network_output, init_state, alphabet, qstring=False, qscale=1.0, qbias=0.0):
    """Mirrors src/lib.rs:214-250 -> search.rs:385-423."""
    x = _as_f32(network_output, 3, "network_output")
    init = _as_f32(init_state, 1, "init_state")
    alpha = _seq_to_vec(alphabet)
    _check_greedy_alphabet(len(alpha), x.shape[2])
    if x.size == 0 or init.size == 0:
        raise RuntimeError("network_output/init_state is empty (the reference asserts and aborts here)")
    x = _dense(x)
    init = np.ascontiguousarray(init)
    out = _HostOut(1, x.shape[0], want_qual=bool(qstring))
    b = _host_batch(x[None], True)
    co = _coalescer
    if co is not None:
        with co:
            co.check(co.lib.fcd_coalescer_crf_greedy_search(co.ptr, C.byref(b), init.ctypes.data, init.shape[0],
                                                            C.byref(out.res)))
    else:
        h = nat.default_handle()
        h.check(h.lib.fcd_crf_greedy_search_host(h.ptr, C.byref(b), init.ctypes.data, init.shape[0],
                                                 init.shape[0], C.byref(out.res)))
    _raise_status(int(out.status[0]))
    n = int(out.out_len[0])
    seq = "".join(alpha[l] for l in out.labels[0, :n])
    if qstring:
        seq += _qual_chars(out.qual[0, :n], qscale, qbias)
    return seq, [int(p) for p in out.path[0, :n]]


def crf_greedy_search_batch_raw(network_outputs, init_states, lengths=None, qual=False):
    """(B,T,S,N) posteriors (numpy or torch ROCm tensor) + (B,n_init) initial state scores ->
    BatchResult of search::crf_greedy_search (src/search.rs:385-423) per read."""
    if _is_torch_cuda(network_outputs):
        import torch
        init = torch.as_tensor(init_states, dtype=torch.float32, device=network_outputs.device).contiguous()
        r = _torch_call("fcd_crf_greedy_search_dev", network_outputs, True, lengths,
                        (C.c_void_p(init.data_ptr()), int(init.shape[1]), int(init.shape[1])), want_qual=qual)
        r._keep = r._keep + (init,)
        return r
    x = _stack_host(network_outputs, 4)
    init = np.ascontiguousarray(np.asarray(init_states, np.float32))
    B, T, S, N = x.shape
    if init.ndim != 2 or init.shape[0] != B:
        raise ValueError("init_states must have shape (n_reads, n_init)")
    h = nat.default_handle()
    out = _HostOut(B, T, want_qual=qual)
    b = _host_batch(x, True, _np_lengths(lengths, B))
    h.check(h.lib.fcd_crf_greedy_search_host(h.ptr, C.byref(b), init.ctypes.data, init.shape[1],
                                             init.shape[1], C.byref(out.res)))
    return BatchResult(out.labels, out.path, out.out_len, out.status, out.qual)


def crf_greedy_search_batch(network_outputs, init_states, alphabet, qstring=False, qscale=1.0, qbias=0.0,
                            lengths=None, paths="list"):
    """Batched crf_greedy_search: element i equals crf_greedy_search(network_outputs[i], init_states[i], ...)."""
    if _device_tensor(network_outputs) is None:
        return _compiled().crf_greedy_search_batch(_host_input(network_outputs), np.asarray(init_states, np.float32),
                                                   alphabet, bool(qstring), qscale, qbias, lengths, paths)
    alpha = _seq_to_vec(alphabet)
    _check_greedy_alphabet(len(alpha), network_outputs.shape[-1])
    r = crf_greedy_search_batch_raw(network_outputs, init_states, lengths, qual=qstring).cpu()
    res = r.sequences(alpha, paths=paths if paths is not None else "array")
    if qstring:
        res = [(s + _qual_chars(r.qual[i, :len(p)], qscale, qbias), p) for i, (s, p) in enumerate(res)]
    return res


def crf_viterbi_search(network_output, init_state, alphabet, qstring=False, qscale=1.0, qbias=0.0):
    """The single most probable path through the CRF model's states over ALL labellings (include/fcd.h,
    fcd_crf_viterbi_search_*; not a reference function) -> (seq, path), crf_greedy_search's arguments, validation and
    messages.  qstring=True appends the phred characters of the emissions' posteriors, as crf_greedy_search does."""
    x = _as_f32(network_output, 3, "network_output")
    init = _as_f32(init_state, 1, "init_state")
    alpha = _seq_to_vec(alphabet)
    _check_greedy_alphabet(len(alpha), x.shape[2])
    if x.size == 0 or init.size == 0:
        raise RuntimeError("network_output/init_state is empty (the reference asserts and aborts here)")
    x = _dense(x)
    init = np.ascontiguousarray(init)
    out = _HostOut(1, x.shape[0], want_qual=bool(qstring))
    b = _host_batch(x[None], True)
    h = nat.default_handle()
    h.check(h.lib.fcd_crf_viterbi_search_host(h.ptr, C.byref(b), init.ctypes.data, init.shape[0], init.shape[0],
                                              C.byref(out.res), None))
    _raise_status(int(out.status[0]))
    n = int(out.out_len[0])
    seq = "".join(alpha[l] for l in out.labels[0, :n])
    if qstring:
        seq += _qual_chars(out.qual[0, :n], qscale, qbias)
    return seq, [int(p) for p in out.path[0, :n]]


def crf_viterbi_search_batch_raw(network_outputs, init_states, lengths=None, qual=False, input_dtype=None):
    """(B,T,S,N) posteriors (numpy float32 / float16 / bfloat16 bits, or a torch ROCm tensor) + (B,n_init) initial state
    scores -> the CRF searches' batch result (so .crf_score / .crf_align / .crf_posterior / .crf_edits work on it) of the
    Viterbi search per read, with .logp: (B,) float64, ln of the path's probability.  Device inputs are enqueued on
    torch's current stream and nothing waits."""
    if _is_torch_cuda(network_outputs):
        import torch
        init = torch.as_tensor(init_states, dtype=torch.float32, device=network_outputs.device).contiguous()
        if init.ndim != 2 or init.shape[0] != network_outputs.shape[0]:
            raise ValueError("init_states must have shape (n_reads, n_init)")
        logp = torch.empty((network_outputs.shape[0],), dtype=torch.float64, device=network_outputs.device)
        r = _torch_call("fcd_crf_viterbi_search_dev", network_outputs, True, lengths,
                        (C.c_void_p(init.data_ptr()), int(init.shape[1]), int(init.shape[1])), want_qual=qual,
                        tail_args=(C.c_void_p(logp.data_ptr()),))
        res = _CrfViterbiResult(r.labels, r.path, r.out_len, r.status, r.qual, logp=logp)
        res._handle = r._handle
        res._keep = r._keep + (init,)
        res._handle.hold_in_flight(init, logp)
        return res
    x = _stack_host(network_outputs, 4)
    init = np.ascontiguousarray(np.asarray(init_states, np.float32))
    B, T, S, N = x.shape
    if init.ndim != 2 or init.shape[0] != B:
        raise ValueError("init_states must have shape (n_reads, n_init)")
    h = nat.default_handle()
    out = _HostOut(B, T, want_qual=qual)
    logp = np.zeros(B, np.float64)
    b = _host_batch(x, True, _np_lengths(lengths, B), input_dtype)
    h.check(h.lib.fcd_crf_viterbi_search_host(h.ptr, C.byref(b), init.ctypes.data, init.shape[1], init.shape[1],
                                              C.byref(out.res), logp.ctypes.data))
    return _CrfViterbiResult(out.labels, out.path, out.out_len, out.status, out.qual, logp=logp)


def crf_viterbi_search_batch(network_outputs, init_states, alphabet, qstring=False, qscale=1.0, qbias=0.0,
                             lengths=None, paths="list"):
    """Batched crf_viterbi_search: element i equals crf_viterbi_search(network_outputs[i], init_states[i], ...)."""
    alpha = _seq_to_vec(alphabet)
    x = network_outputs if _device_tensor(network_outputs) is not None else _stack_host(network_outputs, 4)
    _check_greedy_alphabet(len(alpha), x.shape[-1])
    r = crf_viterbi_search_batch_raw(x, init_states, lengths, qual=bool(qstring)).cpu()
    res = BatchResult.sequences(r, alpha, paths=paths if paths is not None else "array")
    if qstring:
        res = [(s + _qual_chars(r.qual[i, :len(p)], qscale, qbias), p) for i, (s, p) in enumerate(res)]
    if paths is None:
        res = [(s, None) for s, _ in res]
    return res


class TransitionResult:
    """crf_transition_probs_batch_raw's result: probs (B, T, S, N) transition posteriors (float32 or float16; a view of a
    (T, B, S, N) array under time_major_out), init (B, S) float32, logz (B,) float64 (NaN for a failed read) and status
    (B,) int32 -- numpy arrays, or torch tensors on the input's device.  probs and init are what every CRF entry point
    takes as network_outputs and init_states."""

    def __init__(self, probs, init, logz, status):
        self.probs, self.init, self.logz, self.status = probs, init, logz, status

    def cpu(self):
        """-> a TransitionResult of numpy arrays (device results: waits for them)"""
        if isinstance(self.status, np.ndarray):
            return self
        return TransitionResult(*(v.cpu().numpy() for v in (self.probs, self.init, self.logz, self.status)))


_LAYOUT_CODES = {"source": nat.LAYOUT_SOURCE, "dest": nat.LAYOUT_DEST}


def crf_transition_probs_batch_raw(scores, lengths=None, layout="source", out_dtype="float32", input_dtype=None,
                                   time_major_out=False):
    """(B,T,S,N) raw CRF scores -- a network's unnormalised log scores: numpy float32 / float16 / bfloat16 bits, or a torch
    ROCm tensor, any strides (a permuted (T,B,S,N) tensor included) -> TransitionResult: the locally normalised transition
    posteriors and the init row that every CRF entry point takes (include/fcd.h, fcd_crf_transition_probs_*: a backward
    pass over all labellings and a local softmax, on the device).

    layout: "source", scores[b][t][s][a] indexed by the state being left, as the result is; "dest", indexed by the state
    being entered: scores[b][t][s'][0] stays, scores[b][t][s'][1 + i] enters s' from s' // (N-1) + i * (S // (N-1)).
    out_dtype: "float32" or "float16" (the float32 value rounded to nearest; the searches read it as it is).
    time_major_out: probs is stored as (T,B,S,N) and returned as its (B,T,S,N) view.  Rows at and beyond lengths[b] are
    not written (zeros in a numpy result, uninitialised in a torch one).
    Device tensors in: torch tensors out, enqueued on torch's current stream, nothing waits.  numpy in: numpy out."""
    if layout not in _LAYOUT_CODES:
        raise ValueError("layout must be 'source' or 'dest'")
    if out_dtype not in ("float32", "float16"):
        raise ValueError("out_dtype must be 'float32' or 'float16'")
    code = nat.DTYPE_F32 if out_dtype == "float32" else nat.DTYPE_F16
    if _is_torch_cuda(scores):
        import torch
        x = scores
        if x.ndim != 4:
            raise TypeError("expected a tensor of rank 4")
        dcode = _torch_dtype_code(x)
        B, T, S, N = x.shape
        st = x.stride()
        if any(s < 0 for s in st):
            raise ValueError("negative strides: pass a contiguous copy")
        h = nat.default_handle(x.device.index or 0)
        b = nat.Batch(x.data_ptr(), B, T, S, N, st[0], st[1], st[2], st[3], None, dcode)
        if lengths is not None:
            lengths = torch.as_tensor(lengths, dtype=torch.int64, device=x.device).contiguous()
            if tuple(lengths.shape) != (B,):
                raise ValueError("lengths must have shape (n_reads,)")
            b.lengths = lengths.data_ptr()
        tdt = torch.float32 if code == nat.DTYPE_F32 else torch.float16
        buf = torch.empty((T, B, S, N) if time_major_out else (B, T, S, N), dtype=tdt, device=x.device)
        probs = buf.permute(1, 0, 2, 3) if time_major_out else buf
        init = torch.empty((B, S), dtype=torch.float32, device=x.device)
        logz = torch.empty((B,), dtype=torch.float64, device=x.device)
        status = torch.empty((B,), dtype=torch.int32, device=x.device)
        out = nat.Transitions(buf.data_ptr(), code, probs.stride(0) if B * T else S * N, probs.stride(1) if B * T else S * N,
                              init.data_ptr(), S, logz.data_ptr(), status.data_ptr())
        h.set_stream(torch.cuda.current_stream(x.device).cuda_stream)
        h.check(h.lib.fcd_crf_transition_probs_dev(h.ptr, C.byref(b), _LAYOUT_CODES[layout], C.byref(out)))
        h.hold_in_flight(x, lengths, buf, init, logz, status)
        return TransitionResult(probs, init, logz, status)
    x = _stack_host(scores, 4)
    B, T, S, N = x.shape
    h = nat.default_handle()
    b = _host_batch(x, True, _np_lengths(lengths, B), input_dtype)
    ndt = np.float32 if code == nat.DTYPE_F32 else np.float16
    buf = np.zeros((T, B, S, N) if time_major_out else (B, T, S, N), ndt)
    probs = buf.transpose(1, 0, 2, 3) if time_major_out else buf
    init = np.zeros((B, S), np.float32)
    logz = np.zeros(B, np.float64)
    status = np.zeros(B, np.int32)
    sr, stt = (S * N, B * S * N) if time_major_out else (T * S * N, S * N)
    out = nat.Transitions(buf.ctypes.data, code, max(sr, S * N), max(stt, S * N), init.ctypes.data, S, logz.ctypes.data,
                          status.ctypes.data)
    h.check(h.lib.fcd_crf_transition_probs_host(h.ptr, C.byref(b), _LAYOUT_CODES[layout], C.byref(out)))
    return TransitionResult(probs, init, logz, status)


def crf_transition_probs(scores, layout="source"):
    """One read: (T,S,N) raw CRF scores -> (probs (T,S,N) float32, init (S,) float32, logz float) -- what crf_greedy_search,
    crf_beam_search and crf_viterbi_search take as network_output and init_state (crf_transition_probs_batch_raw has the
    definition).  RuntimeError with the status string for a read that fails (a NaN or +inf score, or no path of positive
    weight)."""
    x = _as_f32(scores, 3, "scores")
    r = crf_transition_probs_batch_raw(_dense(x)[None], layout=layout)
    _raise_status(int(r.status[0]))
    return r.probs[0], r.init[0], float(r.logz[0])


class MarginalResult:
    """crf_marginals_batch_raw's result: marginals (B, T, S, N) float32 edge marginals, source-indexed (a view of a
    (T, B, S, N) array under time_major_out), emit (B, T, N) float32 label posteriors per row (None without emit), logz (B,)
    float64 (NaN for a failed read) and status (B,) int32 -- numpy arrays, or torch tensors on the input's device."""

    def __init__(self, marginals, emit, logz, status):
        self.marginals, self.emit, self.logz, self.status = marginals, emit, logz, status

    def cpu(self):
        """-> a MarginalResult of numpy arrays (device results: waits for them)"""
        if isinstance(self.status, np.ndarray):
            return self
        return MarginalResult(*(None if v is None else v.cpu().numpy() for v in (self.marginals, self.emit, self.logz, self.status)))


def _crf_marginals_torch(x, lengths, layout, emit, time_major_out, zeroed=False):
    """the device call on a rank-4 torch ROCm tensor -> (marginals, emit, logz, status), enqueued on the current stream"""
    import torch
    dcode = _torch_dtype_code(x)
    B, T, S, N = x.shape
    st = x.stride()
    if any(s < 0 for s in st):
        raise ValueError("negative strides: pass a contiguous copy")
    h = nat.default_handle(x.device.index or 0)
    b = nat.Batch(x.data_ptr(), B, T, S, N, st[0], st[1], st[2], st[3], None, dcode)
    if lengths is not None:
        lengths = torch.as_tensor(lengths, dtype=torch.int64, device=x.device).contiguous()
        if tuple(lengths.shape) != (B,):
            raise ValueError("lengths must have shape (n_reads,)")
        b.lengths = lengths.data_ptr()
    alloc = torch.zeros if zeroed else torch.empty
    buf = alloc((T, B, S, N) if time_major_out else (B, T, S, N), dtype=torch.float32, device=x.device)
    marg = buf.permute(1, 0, 2, 3) if time_major_out else buf
    em = alloc((B, T, N), dtype=torch.float32, device=x.device) if emit else None
    logz = torch.empty((B,), dtype=torch.float64, device=x.device)
    status = torch.empty((B,), dtype=torch.int32, device=x.device)
    out = nat.Marginals(buf.data_ptr(), marg.stride(0) if B * T else S * N, marg.stride(1) if B * T else S * N,
                        em.data_ptr() if emit else None, T * N, logz.data_ptr(), status.data_ptr())
    h.set_stream(torch.cuda.current_stream(x.device).cuda_stream)
    h.check(h.lib.fcd_crf_marginals_dev(h.ptr, C.byref(b), _LAYOUT_CODES[layout], C.byref(out)))
    h.hold_in_flight(x, lengths, buf, em, logz, status)
    return marg, em, logz, status


def crf_marginals_batch_raw(scores, lengths=None, layout="source", input_dtype=None, emit=True, time_major_out=False):
    """(B,T,S,N) raw CRF scores, as crf_transition_probs_batch_raw takes them -> MarginalResult: the edge marginals over all
    labellings (include/fcd.h, fcd_crf_marginals_*: the backward pass of crf_transition_probs and a forward pass over its
    result, one kernel launch).  marginals[b][t][s][a] is the probability that the model leaves state s by symbol a at row
    t, which is d logz[b] / d scores[b][t][s][a]; emit[b][t][a] is its sum over states, a (T, N) matrix of label posteriors
    whose rows sum to 1.  logz and status are crf_transition_probs_batch_raw's, bit for bit.

    layout: of the scores, "source" or "dest"; the result is always source-indexed.  emit=False: no emit array.
    time_major_out: marginals is stored as (T,B,S,N) and returned as its (B,T,S,N) view.  Rows at and beyond lengths[b]
    are not written (zeros in a numpy result, uninitialised in a torch one).
    Device tensors in: torch tensors out, enqueued on torch's current stream, nothing waits.  numpy in: numpy out."""
    if layout not in _LAYOUT_CODES:
        raise ValueError("layout must be 'source' or 'dest'")
    if _is_torch_cuda(scores):
        if scores.ndim != 4:
            raise TypeError("expected a tensor of rank 4")
        return MarginalResult(*_crf_marginals_torch(scores, lengths, layout, emit, time_major_out))
    x = _stack_host(scores, 4)
    B, T, S, N = x.shape
    h = nat.default_handle()
    b = _host_batch(x, True, _np_lengths(lengths, B), input_dtype)
    buf = np.zeros((T, B, S, N) if time_major_out else (B, T, S, N), np.float32)
    marg = buf.transpose(1, 0, 2, 3) if time_major_out else buf
    em = np.zeros((B, T, N), np.float32) if emit else None
    logz = np.zeros(B, np.float64)
    status = np.zeros(B, np.int32)
    sr, stt = (S * N, B * S * N) if time_major_out else (T * S * N, S * N)
    out = nat.Marginals(buf.ctypes.data, max(sr, S * N), max(stt, S * N), em.ctypes.data if emit else None, T * N,
                        logz.ctypes.data, status.ctypes.data)
    h.check(h.lib.fcd_crf_marginals_host(h.ptr, C.byref(b), _LAYOUT_CODES[layout], C.byref(out)))
    return MarginalResult(marg, em, logz, status)


def crf_marginals(scores, layout="source"):
    """One read: (T,S,N) raw CRF scores -> (marginals (T,S,N) float32, emit (T,N) float32, logz float)
    (crf_marginals_batch_raw has the definition).  RuntimeError with the status string for a read that fails (a NaN or +inf
    score, or no path of positive weight)."""
    x = _as_f32(scores, 3, "scores")
    r = crf_marginals_batch_raw(_dense(x)[None], layout=layout)
    _raise_status(int(r.status[0]))
    return r.marginals[0], r.emit[0], float(r.logz[0])


_CRF_LOGZ_FN = []


def _crf_logz_function():
    if _CRF_LOGZ_FN:
        return _CRF_LOGZ_FN[0]
    import torch

    class CrfLogZ(torch.autograd.Function):
        @staticmethod
        def forward(ctx, scores, lengths):
            # (zeroed: the kernel does not write rows at and beyond a read's length, and the gradient there is 0)
            marg, _, logz, status = _crf_marginals_torch(scores.detach(), lengths, "source", False, False, zeroed=lengths is not None)
            ctx.save_for_backward(marg, status)
            ctx.scores_dtype = scores.dtype
            return logz

        @staticmethod
        def backward(ctx, grad_logz):
            marg, status = ctx.saved_tensors
            g = grad_logz.to(torch.float32)[:, None, None, None] * marg
            g = torch.where((status != 0)[:, None, None, None], torch.full_like(g, float("nan")), g)  # (selected on the device)
            return g.to(ctx.scores_dtype), None

    _CRF_LOGZ_FN.append(CrfLogZ.apply)
    return CrfLogZ.apply


def crf_logz(scores, lengths=None):
    """(B,T,S,N) raw CRF scores, a torch ROCm tensor (float32 / float16 / bfloat16, any non-negative strides) in the
    "source" layout -> logz (B,) float64, differentiable: the denominator of CRF-CTC training.  Its backward pass is
    grad_out[:, None, None, None] * marginals (crf_marginals_batch_raw) in the dtype of `scores` -- the forward call has
    already computed them, in the same kernel launch; rows at and beyond lengths[b] get gradient 0, a failed read (logz
    NaN) a NaN gradient.  Nothing synchronises.  Out of scope: the "dest" layout.  The numerator of a training loss -- a
    labelling's own score and its gradient -- is crf_occupancy_batch_raw's, and crf_ctc_loss is the whole loss."""
    if not _is_torch_cuda(scores):
        raise TypeError("crf_logz takes a torch ROCm tensor")
    if scores.ndim != 4:
        raise TypeError("expected a tensor of rank 4")
    return _crf_logz_function()(scores, lengths)


_CRF_CTC_LOSS_FN = []


def _crf_ctc_loss_function():
    if _CRF_CTC_LOSS_FN:
        return _CRF_CTC_LOSS_FN[0]
    import torch

    class CrfCtcLoss(torch.autograd.Function):
        @staticmethod
        def forward(ctx, scores, labels, label_lengths, lengths, start_states):
            x = scores.detach()
            tr = crf_transition_probs_batch_raw(x, lengths)
            # (zeroed: neither launch writes rows at and beyond a read's length, and the gradient there is 0)
            grad, _, _, status = _crf_marginals_torch(x, lengths, "source", False, False, zeroed=lengths is not None)
            if start_states is None:
                init, start = tr.init, tr.init.max(dim=1).values  # (sigma_0: the first maximum, as every CRF walk takes it)
            else:
                at = torch.as_tensor(start_states, device=x.device).to(torch.int64).reshape(-1, 1)
                init = torch.zeros_like(tr.init).scatter_(1, at, 1.0)
                start = tr.init.gather(1, at)[:, 0]
            # grad = marginals - occupancy, the gradient of logz - ln(sum over the labelling's alignments of exp(score))
            occ = crf_occupancy_batch_raw(tr.probs, init, labels, label_lengths, lengths, out=grad, scale=-1.0, accumulate=True,
                                          wide=True)
            logp = occ.logp[:, 0]
            loss = -(logp + torch.log(start.to(torch.float64)))
            # (a labelling whose lattice the occupancy walk gave up comes back with logp NaN: its loss and gradient are NaN)
            loss = torch.where(status != 0, torch.full_like(loss, float("nan")), loss)  # (selected on the device)
            ctx.save_for_backward(grad, status, logp)
            ctx.scores_dtype = scores.dtype
            return loss

        @staticmethod
        def backward(ctx, grad_loss):
            grad, status, logp = ctx.saved_tensors
            g = grad_loss.to(torch.float32)[:, None, None, None] * grad
            bad = (status != 0) | ~torch.isfinite(logp)
            g = torch.where(bad[:, None, None, None], torch.full_like(g, float("nan")), g)  # (selected on the device)
            return g.to(ctx.scores_dtype), None, None, None, None

    _CRF_CTC_LOSS_FN.append(CrfCtcLoss.apply)
    return CrfCtcLoss.apply


def crf_ctc_loss(scores, labels, label_lengths, lengths=None, start_states=None):
    """The CRF-CTC training loss.  scores: (B,T,S,N) raw CRF scores, a torch ROCm tensor (float32 / float16 / bfloat16) in
    the "source" layout; labels (B, Lmax) uint8 with values 1 .. N-1, label_lengths (B,); lengths (B,) rows per read.
    -> loss (B,) float64, differentiable:  loss_b = -ln P(y_b, sigma_0 | x_b) = logz - ln(sum over the alignments of y_b from
    sigma_0 of exp(score)).  sigma_0 is the model's most probable start state (the first maximum of the init row
    crf_transition_probs_batch_raw returns), or start_states[b] ((B,) integers in 0 .. S-1) where given.

    Forward: crf_transition_probs_batch_raw (posteriors, init, logz), crf_marginals_batch_raw (the gradient of logz) and
    crf_occupancy_batch_raw, which subtracts the labelling's edge occupancies from the marginals in place and returns
    ln P(y | x, sigma_0).  Backward: grad_out[:, None, None, None] * (marginals - occupancy) in the dtype of `scores`; 0 on
    rows at and beyond lengths[b]; NaN for a read whose scores fail (loss NaN), whose labelling has no alignment (loss
    +inf: more labels than rows) or whose lattice the walk gave up (loss NaN).  Nothing synchronises.
    The lattice walks keep one float32 exponent per row.  A long read that does not support its labelling (near-uniform or
    random scores against a labelling with many rows per label, as an untrained network gives on a long chunk) puts the
    forward and backward maxima at opposite ends of the lattice and the cells that carry the probability out of range.  The
    occupancy walk checks every row's terms against 1 and gives such a labelling up: its loss and gradient are NaN, not
    wrong.  Chunks of 600 to 1000 rows with about half as many labels are inside the range (INTEGRATION.md section 2m has the
    measured boundary); train on chunks of that size.
    Cost of composing existing launches: the backward pass over all labellings runs twice (once for the posteriors, once
    inside the marginals launch), and two (B,T,S,N) float32 buffers are held (the posteriors until the call returns, the
    gradient until backward).  Limits: crf_occupancy_batch_raw's with wide=True, exact lattice: labellings up to 4095 rows
    or labels at N - 1 <= 8 whose copy, tile, window rows and S * N row fit the 160 KiB of LDS (S = 1024 and S = 4096 at
    N = 5: 2047 labels and more).  Up to 511 labels the register-resident walks run, as before; beyond, the LDS-resident
    ones."""
    if not _is_torch_cuda(scores):
        raise TypeError("crf_ctc_loss takes a torch ROCm tensor")
    if scores.ndim != 4:
        raise TypeError("expected a tensor of rank 4")
    if getattr(labels, "ndim", 2) != 2:
        raise ValueError("labels must have shape (n_reads, Lmax): one labelling per read")
    return _crf_ctc_loss_function()(scores, labels, label_lengths, lengths, start_states)


_DEFAULT_LOGADD = [nat.LOGADD_LOGSUMEXP]


_MODE_CODES = {"logsumexp": nat.LOGADD_LOGSUMEXP, "max": nat.LOGADD_MAX, "logsumexp_glibc235": nat.LOGADD_LOGSUMEXP_GLIBC235,
               nat.LOGADD_LOGSUMEXP: nat.LOGADD_LOGSUMEXP, nat.LOGADD_MAX: nat.LOGADD_MAX,
               nat.LOGADD_LOGSUMEXP_GLIBC235: nat.LOGADD_LOGSUMEXP_GLIBC235}


def set_duplex_logadd_mode(mode):
    """Select the duplex log-space addition: "logsumexp" (the reference built with
    --no-default-features; BASELINE.json's north star; ln / exp / ln_1p correctly rounded), "max" (the reference's
    default `fastexp` feature, whose exp() is identically 0.0 -- what the PyPI wheels compute; SURVEY.md finding 3) or
    "logsumexp_glibc235" (logsumexp on glibc 2.35's expf / logf / log1pf, bit for bit: what the reference computes on
    such a host -- csrc/glibc235_math.h)."""
    _DEFAULT_LOGADD[0] = _MODE_CODES[mode]


def set_tie_order(order):
    """How the beam searches order EQUAL probabilities among more than 20 candidates: "pdq178" (default: what Rust
    1.78's sort_unstable_by -- the reference wheels' toolchain -- leaves them in) or "stable" (ascending node index).
    Process-wide; the same switch as the compiled module's set_tie_order and the C ABI's fcd_set_default_tie_order."""
    nat.set_default_tie_order(order)


def tie_order():
    return nat.default_tie_order()


def set_overlap(streams, device=0):
    """Device-tensor batches only: let successive beam_search_batch_raw / crf_beam_search_batch_raw calls of this thread
    overlap on `streams` (2 .. 8) internal HIP streams of the thread's handle (include/fcd.h, fcd_set_overlap).  A batch is
    as slow as its slowest read and 4096 reads fill half the chip, so independent batches issued back to back finish
    sooner when they share it (BASELINE config 2: 0.94 M -> 1.4 M reads/s; config 3 under the default tie order: 141 k ->
    300 k).  Each call still starts behind everything torch's current stream held when it was made; a result is
    complete when its `.cpu()` / `.sequences()` has run (they join first) or after overlap_join().  0 = off (default)."""
    nat.default_handle(device).set_overlap(streams)


def overlap_join(device=0):
    """torch's current stream waits for every overlapping call made so far (set_overlap)."""
    import torch
    h = nat.default_handle(device)
    h.set_stream(torch.cuda.current_stream(device).cuda_stream)
    h.overlap_join()


import os as _os
if _os.environ.get("FCD_DUPLEX_LOGADD"):   # the same switch the compiled module reads at import
    set_duplex_logadd_mode(_os.environ["FCD_DUPLEX_LOGADD"])


def _check_envelope(envelope, T1):
    """src/lib.rs:445-456"""
    if envelope is None:
        return
    if not isinstance(envelope, np.ndarray) or envelope.dtype != np.uint64 or envelope.ndim != 2:
        raise TypeError("argument 'envelope': expected a 2-dimensional uint64 array")
    if envelope.shape[0] != T1:
        raise ValueError("the lengths of network_output_1 and envelope do not match")
    if envelope.shape[1] != 2:
        raise ValueError("the inner axis of envelope must have size 2")


def _default_envelope(B, T1, T2, lengths_2=None):
    """src/lib.rs:459-468: every row searches the whole of read 2 -- of THAT pair's read 2 when the
    batch is ragged (an upper bound past the pair's own T2 is an out-of-range slice in the reference)."""
    env = np.empty((B, max(T1, 1), 2), np.uint64)
    env[:, :, 0] = 0
    if lengths_2 is None:
        env[:, :, 1] = T2
    else:
        l2 = np.asarray(lengths_2.cpu() if hasattr(lengths_2, "cpu") else lengths_2, np.int64)
        env[:, :, 1] = np.clip(l2, 0, T2).astype(np.uint64)[:, None]
    return env


def beam_search_duplex_batch_raw(network_outputs_1, network_outputs_2, envelopes=None, beam_size=5,
                                 beam_cut_threshold=0.0, collapse_repeats=True, lengths_1=None,
                                 lengths_2=None, logadd_mode=None, count_ambiguous=False):
    """(B,T1,N) and (B,T2,N) posteriors + (B,T1,2) uint64 envelopes -> BatchResult (labels only).
    `count_ambiguous`: also fill BatchResult.ambiguous, the tie counters of the prune (include/fcd.h)."""
    mode = _DEFAULT_LOGADD[0] if logadd_mode is None else _MODE_CODES[logadd_mode]
    if _is_torch_cuda(network_outputs_1):
        import torch
        x1, x2 = network_outputs_1, network_outputs_2
        d1, d2 = _torch_dtype_code(x1), _torch_dtype_code(x2)
        B, T1, N = x1.shape
        T2 = x2.shape[1]
        dev = x1.device
        if envelopes is None:
            env = torch.from_numpy(_default_envelope(B, T1, T2, lengths_2).view(np.int64)).to(dev)
        elif isinstance(envelopes, np.ndarray):
            env = torch.from_numpy(np.ascontiguousarray(envelopes, np.uint64).view(np.int64)).to(dev)
        else:
            env = envelopes.contiguous()  # int64 tensor holding the u64 bit patterns
        h = nat.default_handle(dev.index or 0)
        s1, s2 = x1.stride(), x2.stride()
        b1 = nat.Batch(x1.data_ptr(), B, T1, 1, N, s1[0], s1[1], 0, s1[2], None, d1)
        b2 = nat.Batch(x2.data_ptr(), B, T2, 1, N, s2[0], s2[1], 0, s2[2], None, d2)
        keep = [x1, x2, env]
        if lengths_1 is not None:
            l1 = torch.as_tensor(lengths_1, dtype=torch.int64, device=dev).contiguous()
            b1.lengths = l1.data_ptr()
            keep.append(l1)
        if lengths_2 is not None:
            l2 = torch.as_tensor(lengths_2, dtype=torch.int64, device=dev).contiguous()
            b2.lengths = l2.data_ptr()
            keep.append(l2)
        w = max(int(T1), 1)
        labels = torch.empty((B, w), dtype=torch.uint8, device=dev)
        out_len = torch.zeros(B, dtype=torch.int32, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        amb = torch.zeros((B, 2), dtype=torch.int32, device=dev) if count_ambiguous else None
        res = nat.Result(labels.data_ptr(), None, None, out_len.data_ptr(), status.data_ptr(), w,
                         amb.data_ptr() if count_ambiguous else None)
        h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        h.check(h.lib.fcd_beam_search_duplex_dev(
            h.ptr, C.byref(b1), C.byref(b2), C.c_void_p(env.data_ptr()), int(env.shape[1]),
            int(beam_size), float(beam_cut_threshold), int(bool(collapse_repeats)), int(mode),
            C.byref(res)))
        r = BatchResult(labels, None, out_len, status, ambiguous=amb)
        r._handle, r._keep = h, keep
        h.hold_in_flight(keep, labels, out_len, status, amb)
        return r
    x1 = _stack_host(network_outputs_1, 3)
    x2 = _stack_host(network_outputs_2, 3)
    B, T1, N = x1.shape
    T2 = x2.shape[1]
    if x2.shape[0] != B:
        raise ValueError("both batches must hold the same number of reads")
    env = _default_envelope(B, T1, T2, lengths_2) if envelopes is None else np.ascontiguousarray(envelopes, np.uint64)
    if env.shape[0] != B or env.ndim != 3 or env.shape[2] != 2 or env.shape[1] < T1:
        raise ValueError("envelopes must have shape (n_pairs, T1, 2)")
    h = nat.default_handle()
    out = _HostOut(B, T1, want_path=False, want_amb=count_ambiguous)
    l1, l2 = _np_lengths(lengths_1, B), _np_lengths(lengths_2, B)
    b1, b2 = _host_batch(x1, False, l1), _host_batch(x2, False, l2)
    h.check(h.lib.fcd_beam_search_duplex_host(
        h.ptr, C.byref(b1), C.byref(b2), env.ctypes.data, int(env.shape[1]), int(beam_size),
        float(beam_cut_threshold), int(bool(collapse_repeats)), int(mode), C.byref(out.res)))
    r = BatchResult(out.labels, None, out.out_len, out.status, ambiguous=out.ambiguous)
    r._handle = h
    return r


def beam_search_duplex(network_output_1, network_output_2, alphabet, envelope=None, beam_size=5,
                       beam_cut_threshold=0.0, collapse_repeats=True, *, logadd_mode=None):
    """Mirrors src/lib.rs:401-488 -> duplex.rs:443-650.  Returns the consensus sequence (str).
    `logadd_mode` (keyword-only, not a reference argument) overrides set_duplex_logadd_mode()."""
    x1 = _as_f32(network_output_1, 2, "network_output_1")
    x2 = _as_f32(network_output_2, 2, "network_output_2")
    alpha = _seq_to_vec(alphabet)
    if x1.shape[1] != x2.shape[1]:
        raise ValueError("inner axes of the network outputs do not match")
    _check_beam_args(len(alpha), x1.shape[1], beam_size, beam_cut_threshold)
    _check_envelope(envelope, x1.shape[0])
    if x1.shape[0] == 0:
        raise RuntimeError("network_output_1 is empty (the reference indexes envelope[(0,1)] and aborts)")
    co = _coalescer
    if co is not None:  # concurrent per-pair calls share a launch (set_coalescing; csrc/coalesce.hip)
        mode = _DEFAULT_LOGADD[0] if logadd_mode is None else _MODE_CODES[logadd_mode]
        x1, x2 = _dense(x1), _dense(x2)
        env = (_default_envelope(1, x1.shape[0], x2.shape[0])[0] if envelope is None
               else np.ascontiguousarray(envelope, np.uint64))
        r = _HostOut(1, x1.shape[0], want_path=False)
        b1, b2 = _host_batch(x1[None], False), _host_batch(x2[None], False)
        with co:
            co.check(co.lib.fcd_coalescer_beam_search_duplex(
                co.ptr, C.byref(b1), C.byref(b2), env.ctypes.data, int(beam_size), float(beam_cut_threshold),
                int(bool(collapse_repeats)), int(mode), C.byref(r.res)))
    else:
        env = None if envelope is None else np.ascontiguousarray(envelope)[None]
        r = beam_search_duplex_batch_raw(_dense(x1)[None], _dense(x2)[None], env, beam_size,
                                         beam_cut_threshold, collapse_repeats, logadd_mode=logadd_mode)
    _raise_status(int(r.status[0]))
    n = int(r.out_len[0])
    return "".join(alpha[l] for l in r.labels[0, :n])


def beam_search_duplex_batch(network_outputs_1, network_outputs_2, alphabet, envelopes=None,
                             beam_size=5, beam_cut_threshold=0.0, collapse_repeats=True,
                             lengths_1=None, lengths_2=None, logadd_mode=None):
    """Batched beam_search_duplex -> list[str]."""
    if _device_tensor(network_outputs_1) is None:  # host input: the compiled layer (one host layer, not two)
        mode = int(_DEFAULT_LOGADD[0] if logadd_mode is None else _MODE_CODES[logadd_mode])
        return _compiled().beam_search_duplex_batch(_host_input(network_outputs_1), _host_input(network_outputs_2),
                                                    alphabet, envelopes, beam_size, beam_cut_threshold,
                                                    collapse_repeats, lengths_1, lengths_2, True, mode)
    alpha = _seq_to_vec(alphabet)
    if network_outputs_1.shape[-1] != network_outputs_2.shape[-1]:
        raise ValueError("inner axes of the network outputs do not match")
    _check_beam_args(len(alpha), network_outputs_1.shape[-1], beam_size, beam_cut_threshold)
    r = beam_search_duplex_batch_raw(network_outputs_1, network_outputs_2, envelopes, beam_size,
                                     beam_cut_threshold, collapse_repeats, lengths_1, lengths_2,
                                     logadd_mode).cpu()
    return [s for s, _ in r.sequences(alpha)]


def estimate_envelope_batch(network_outputs_1, network_outputs_2, band=64, lengths_1=None, lengths_2=None):
    """Alignment-band estimator for the duplex searches: (B,T1,N) and (B,T2,N) posteriors ->
    (B,T1,2) envelopes usable as `envelopes=` of beam_search_duplex_batch*.

    NOT a reference function (the reference defaults to the full matrix and only anticipates a
    better default, /root/reference/src/lib.rs:376-378): both reads are decoded greedily
    (viterbi_search), the label sequences are aligned globally on the GPU, matched labels anchor
    read-1 time to read-2 time, and row i becomes [centre(i) - band, centre(i) + band + 1) with the
    rows forced to start at 0, end at T2 and touch (specification: tests/envelope_model.py).
    Device tensors in -> int64 torch tensor holding the u64 bit patterns; numpy in -> uint64 array."""
    if _is_torch_cuda(network_outputs_1):
        import torch
        x1, x2 = network_outputs_1, network_outputs_2
        B, T1 = int(x1.shape[0]), int(x1.shape[1])
        T2 = int(x2.shape[1])
        dev = x1.device
        r1 = viterbi_search_batch_raw(x1, True, lengths_1)
        r2 = viterbi_search_batch_raw(x2, True, lengths_2)
        env = torch.zeros((B, max(T1, 1), 2), dtype=torch.int64, device=dev)
        keep = [r1, r2]
        l1 = l2 = None
        if lengths_1 is not None:
            l1 = torch.as_tensor(lengths_1, dtype=torch.int64, device=dev).contiguous()
        if lengths_2 is not None:
            l2 = torch.as_tensor(lengths_2, dtype=torch.int64, device=dev).contiguous()
        h = r1._handle
        h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        h.check(h.lib.fcd_duplex_envelope_dev(
            h.ptr, B, r1.labels.data_ptr(), r1.path.data_ptr(), r1.out_len.data_ptr(), int(r1.labels.shape[1]),
            None if l1 is None else l1.data_ptr(), T1,
            r2.labels.data_ptr(), r2.path.data_ptr(), r2.out_len.data_ptr(), int(r2.labels.shape[1]),
            None if l2 is None else l2.data_ptr(), T2, int(band), env.data_ptr(), int(env.shape[1])))
        env._keep = (keep, l1, l2)
        return env
    x1 = _stack_host(network_outputs_1, 3)
    x2 = _stack_host(network_outputs_2, 3)
    B, T1, _ = x1.shape
    T2 = x2.shape[1]
    if x2.shape[0] != B:
        raise ValueError("both batches must hold the same number of reads")
    r1 = viterbi_search_batch_raw(x1, True, lengths_1)
    r2 = viterbi_search_batch_raw(x2, True, lengths_2)
    env = np.zeros((B, max(T1, 1), 2), np.uint64)
    l1, l2 = _np_lengths(lengths_1, B), _np_lengths(lengths_2, B)
    h = nat.default_handle()
    lab1, lab2 = np.ascontiguousarray(r1.labels), np.ascontiguousarray(r2.labels)
    p1, p2 = np.ascontiguousarray(r1.path).view(np.uint32), np.ascontiguousarray(r2.path).view(np.uint32)
    n1, n2 = np.ascontiguousarray(r1.out_len).view(np.uint32), np.ascontiguousarray(r2.out_len).view(np.uint32)
    h.check(h.lib.fcd_duplex_envelope_host(
        h.ptr, B, lab1.ctypes.data, p1.ctypes.data, n1.ctypes.data, int(lab1.shape[1]),
        None if l1 is None else l1.ctypes.data, T1,
        lab2.ctypes.data, p2.ctypes.data, n2.ctypes.data, int(lab2.shape[1]),
        None if l2 is None else l2.ctypes.data, T2, int(band), env.ctypes.data, int(env.shape[1])))
    return env[:, :T1]


def estimate_envelope(network_output_1, network_output_2, band=64):
    """Single pair: (T1,N), (T2,N) posteriors -> (T1,2) uint64 envelope for beam_search_duplex(envelope=...)."""
    x1 = np.asarray(network_output_1)
    x2 = np.asarray(network_output_2)
    if x1.ndim != 2 or x2.ndim != 2:
        raise ValueError("expected two (T, N) matrices")
    if x1.shape[0] == 0:
        return np.zeros((0, 2), np.uint64)
    return estimate_envelope_batch(_dense(x1)[None], _dense(x2)[None], band)[0]


def crf_beam_search_duplex_batch_raw(network_outputs_1, init_states_1, network_outputs_2,
                                     init_states_2, envelopes=None, beam_size=5,
                                     beam_cut_threshold=0.0, lengths_1=None, lengths_2=None,
                                     logadd_mode=None, count_ambiguous=False):
    """(B,T1,S,N) / (B,T2,S,N) posteriors (numpy, or torch ROCm tensors: zero-copy), (B,n_init)
    initial state scores, (B,T1,2) uint64 envelopes -> BatchResult (labels only)."""
    mode = _DEFAULT_LOGADD[0] if logadd_mode is None else _MODE_CODES[logadd_mode]
    if _is_torch_cuda(network_outputs_1):
        import torch
        x1, x2 = network_outputs_1, network_outputs_2
        d1, d2 = _torch_dtype_code(x1), _torch_dtype_code(x2)
        B, T1, S, N = x1.shape
        T2 = x2.shape[1]
        dev = x1.device
        i1 = torch.as_tensor(init_states_1, dtype=torch.float32, device=dev).contiguous()
        i2 = torch.as_tensor(init_states_2, dtype=torch.float32, device=dev).contiguous()
        if x2.shape[0] != B or i1.shape[0] != B or i2.shape[0] != B or i1.ndim != 2 or i2.ndim != 2:
            raise ValueError("all inputs must hold the same number of pairs")
        if envelopes is None:
            env = torch.from_numpy(_default_envelope(B, T1, T2, lengths_2).view(np.int64)).to(dev)
        elif isinstance(envelopes, np.ndarray):
            env = torch.from_numpy(np.ascontiguousarray(envelopes, np.uint64).view(np.int64)).to(dev)
        else:
            env = envelopes.contiguous()
        h = nat.default_handle(dev.index or 0)
        s1, s2 = x1.stride(), x2.stride()
        b1 = nat.Batch(x1.data_ptr(), B, T1, S, N, s1[0], s1[1], s1[2], s1[3], None, d1)
        b2 = nat.Batch(x2.data_ptr(), B, T2, S, N, s2[0], s2[1], s2[2], s2[3], None, d2)
        keep = [x1, x2, env, i1, i2]
        if lengths_1 is not None:
            l1 = torch.as_tensor(lengths_1, dtype=torch.int64, device=dev).contiguous()
            b1.lengths = l1.data_ptr()
            keep.append(l1)
        if lengths_2 is not None:
            l2 = torch.as_tensor(lengths_2, dtype=torch.int64, device=dev).contiguous()
            b2.lengths = l2.data_ptr()
            keep.append(l2)
        w = max(int(T1), 1)
        labels = torch.empty((B, w), dtype=torch.uint8, device=dev)
        out_len = torch.zeros(B, dtype=torch.int32, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        amb = torch.zeros((B, 2), dtype=torch.int32, device=dev) if count_ambiguous else None
        res = nat.Result(labels.data_ptr(), None, None, out_len.data_ptr(), status.data_ptr(), w,
                         amb.data_ptr() if count_ambiguous else None)
        h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        h.check(h.lib.fcd_crf_beam_search_duplex_dev(
            h.ptr, C.byref(b1), C.c_void_p(i1.data_ptr()), int(i1.shape[1]), int(i1.shape[1]), C.byref(b2),
            C.c_void_p(i2.data_ptr()), int(i2.shape[1]), int(i2.shape[1]), C.c_void_p(env.data_ptr()),
            int(env.shape[1]), int(beam_size), float(beam_cut_threshold), int(mode), C.byref(res)))
        r = BatchResult(labels, None, out_len, status, ambiguous=amb)
        r._handle, r._keep = h, keep
        h.hold_in_flight(keep, labels, out_len, status, amb)
        return r
    x1 = _stack_host(network_outputs_1, 4)
    x2 = _stack_host(network_outputs_2, 4)
    i1 = np.ascontiguousarray(np.asarray(init_states_1, np.float32))
    i2 = np.ascontiguousarray(np.asarray(init_states_2, np.float32))
    B, T1, S, N = x1.shape
    T2 = x2.shape[1]
    if x2.shape[0] != B or i1.shape[0] != B or i2.shape[0] != B or i1.ndim != 2 or i2.ndim != 2:
        raise ValueError("all inputs must hold the same number of pairs")
    env = _default_envelope(B, T1, T2, lengths_2) if envelopes is None else np.ascontiguousarray(envelopes, np.uint64)
    if env.shape[0] != B or env.ndim != 3 or env.shape[2] != 2 or env.shape[1] < T1:
        raise ValueError("envelopes must have shape (n_pairs, T1, 2)")
    h = nat.default_handle()
    out = _HostOut(B, T1, want_path=False, want_amb=count_ambiguous)
    l1, l2 = _np_lengths(lengths_1, B), _np_lengths(lengths_2, B)
    b1, b2 = _host_batch(x1, True, l1), _host_batch(x2, True, l2)
    h.check(h.lib.fcd_crf_beam_search_duplex_host(
        h.ptr, C.byref(b1), i1.ctypes.data, int(i1.shape[1]), int(i1.shape[1]), C.byref(b2),
        i2.ctypes.data, int(i2.shape[1]), int(i2.shape[1]), env.ctypes.data, int(env.shape[1]),
        int(beam_size), float(beam_cut_threshold), int(mode), C.byref(out.res)))
    r = BatchResult(out.labels, None, out.out_len, out.status, ambiguous=out.ambiguous)
    r._handle = h
    return r


def crf_beam_search_duplex_batch(network_outputs_1, init_states_1, network_outputs_2, init_states_2, alphabet,
                                 envelopes=None, beam_size=5, beam_cut_threshold=0.0, lengths_1=None, lengths_2=None,
                                 logadd_mode=None):
    """Batched crf_beam_search_duplex on HOST arrays -> list[str] (the compiled layer's function)."""
    mode = int(_DEFAULT_LOGADD[0] if logadd_mode is None else _MODE_CODES[logadd_mode])
    return _compiled().crf_beam_search_duplex_batch(_host_input(network_outputs_1), init_states_1,
                                                    _host_input(network_outputs_2), init_states_2, alphabet, envelopes,
                                                    beam_size, beam_cut_threshold, lengths_1, lengths_2, True, mode)


def crf_beam_search_duplex(network_output_1, init_state_1, network_output_2, init_state_2,
                           alphabet, envelope=None, beam_size=5, beam_cut_threshold=0.0, *,
                           logadd_mode=None):
    """Mirrors src/lib.rs:490-578 -> duplex.rs:652-834.  Returns the consensus sequence (str)."""
    x1 = _as_f32(network_output_1, 3, "network_output_1")
    i1 = _as_f32(init_state_1, 1, "init_state_1")
    x2 = _as_f32(network_output_2, 3, "network_output_2")
    i2 = _as_f32(init_state_2, 1, "init_state_2")
    alpha = _seq_to_vec(alphabet)
    if x1.shape[2] != x2.shape[2]:
        raise ValueError("inner axes of the network outputs do not match")
    # src/lib.rs:509-530 (the message quotes shape()[1], as the reference does)
    n_alpha = len(alpha)
    if n_alpha != x1.shape[2]:
        raise ValueError("alphabet size %d does not match probability matrix inner dimension %d"
                         % (n_alpha, x1.shape[1]))
    _check_beam_args(n_alpha, x1.shape[2], beam_size, beam_cut_threshold)
    _check_envelope(envelope, x1.shape[0])
    if x1.shape[1] != x2.shape[1]:
        raise RuntimeError("state axes of the network outputs do not match (the reference asserts and aborts)")
    if x1.shape[0] == 0 or i1.size == 0 or i2.size == 0:
        raise RuntimeError("empty network_output_1 / init_state (the reference aborts here)")
    co = _coalescer
    if co is not None:
        mode = _DEFAULT_LOGADD[0] if logadd_mode is None else _MODE_CODES[logadd_mode]
        x1, x2, i1, i2 = _dense(x1), _dense(x2), np.ascontiguousarray(i1), np.ascontiguousarray(i2)
        env = (_default_envelope(1, x1.shape[0], x2.shape[0])[0] if envelope is None
               else np.ascontiguousarray(envelope, np.uint64))
        r = _HostOut(1, x1.shape[0], want_path=False)
        b1, b2 = _host_batch(x1[None], True), _host_batch(x2[None], True)
        with co:
            co.check(co.lib.fcd_coalescer_crf_beam_search_duplex(
                co.ptr, C.byref(b1), i1.ctypes.data, i1.shape[0], C.byref(b2), i2.ctypes.data, i2.shape[0],
                env.ctypes.data, int(beam_size), float(beam_cut_threshold), int(mode), C.byref(r.res)))
    else:
        env = None if envelope is None else np.ascontiguousarray(envelope)[None]
        r = crf_beam_search_duplex_batch_raw(_dense(x1)[None], np.ascontiguousarray(i1)[None],
                                             _dense(x2)[None], np.ascontiguousarray(i2)[None], env,
                                             beam_size, beam_cut_threshold, logadd_mode=logadd_mode)
    _raise_status(int(r.status[0]))
    n = int(r.out_len[0])
    # src/duplex.rs:825-833: labels appended leaf -> root, then the CHARACTERS reversed
    return "".join(alpha[l] for l in r.labels[0, :n][::-1])[::-1]


# ---------------------------------------------------------------------------------------------
# additive batch API
# ---------------------------------------------------------------------------------------------
def _is_torch_cuda(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda") and bool(x.is_cuda)


def _to_host(a):
    """numpy (and None, and anything that is no device array) as it is; a torch tensor as a numpy array: waits for it"""
    return a if a is None or isinstance(a, np.ndarray) or not hasattr(a, "cpu") else a.cpu().numpy()


class _LatticeMethods:
    """The labelling-lattice calls (ctc_score_batch_raw ... crf_occupancy_batch_raw) on a search result's own arrays, for
    BatchResult (one labelling per read: arrays (n_reads, 1, ...)) and NBestResult (n_hyp as n_valid: arrays
    (n_reads, n_best, ...), and NaN / nothing where i >= n_hyp[r]).  Device results stay on the device: no host round
    trip.  A class says which results it refuses (_lattice_refuses) and which rows count (_lattice_n_valid)."""

    def _lattice(self, model, kind, network_outputs, lengths, band, input_dtype, **kw):
        rank = 4 if model == "crf" else 3
        if self._lattice_refuses(model) or getattr(network_outputs, "ndim", rank) != rank:
            if model == "crf":
                raise ValueError("crf_%s covers the results of the CRF searches, (n_reads, T, S, N) posteriors, not plain CTC results" % kind)
            raise ValueError("ctc_%s covers the plain CTC searches, not CRF results" % kind)
        n_valid = self._lattice_n_valid(band)
        return _lattice_call(model, kind, network_outputs, self.labels, self.out_len, lengths, self.path if band else None,
                             band, n_valid, input_dtype, getattr(self, "_handle", None), **kw)

    def ctc_score(self, network_outputs, collapse_repeats=True, lengths=None, band=0, input_dtype=None):
        """ln P(labelling | posteriors) of every read's result, float64 (n_reads, 1) -- of every hypothesis,
        (n_reads, n_best), NaN where i >= n_hyp[r]: ctc_score_batch_raw on this result's own arrays.  `network_outputs`,
        `lengths` and `collapse_repeats` as given to the search.  A failed read has an empty labelling and scores as one.
        CRF results are refused (transition-scored models: a different lattice)."""
        return self._lattice("ctc", "score", network_outputs, lengths, band, input_dtype, collapse_repeats=collapse_repeats)

    def ctc_align(self, network_outputs, collapse_repeats=True, lengths=None, band=0, input_dtype=None):
        """The best alignment of every read's result to its rows -> AlignResult, arrays (n_reads, 1, stride) -- of every
        hypothesis, (n_reads, n_best, stride), logp NaN and count 0 where i >= n_hyp[r]: ctc_align_batch_raw on this
        result's own arrays.  Arguments as ctc_score.  CRF results are refused."""
        return self._lattice("ctc", "align", network_outputs, lengths, band, input_dtype, collapse_repeats=collapse_repeats)

    def ctc_posterior(self, network_outputs, collapse_repeats=True, lengths=None, band=0, input_dtype=None):
        """The substitution posteriors of every read's result -> PosteriorResult, post (n_reads, 1, stride, N-1) -- of
        every hypothesis, (n_reads, n_best, stride, N-1), logp NaN where i >= n_hyp[r]: ctc_posterior_batch_raw on this
        result's own arrays.  Arguments as ctc_score.  CRF results are refused."""
        return self._lattice("ctc", "posterior", network_outputs, lengths, band, input_dtype, collapse_repeats=collapse_repeats)

    def ctc_edits(self, network_outputs, collapse_repeats=True, lengths=None, band=0, input_dtype=None):
        """The deletion and insertion likelihoods of every read's result -> EditResult, deletion (n_reads, 1, stride),
        insertion (n_reads, 1, stride + 1, N-1) -- of every hypothesis, (n_reads, n_best, stride) and
        (n_reads, n_best, stride + 1, N-1), logp NaN where i >= n_hyp[r]: ctc_edits_batch_raw on this result's own arrays.
        Arguments as ctc_score.  CRF results are refused."""
        return self._lattice("ctc", "edits", network_outputs, lengths, band, input_dtype, collapse_repeats=collapse_repeats)

    def ctc_occupancy(self, network_outputs, collapse_repeats=True, lengths=None, band=0, input_dtype=None, wide=False):
        """The label occupancies of every read's result -> OccupancyResult, occupancy (n_reads, 1, T, N) -- of every
        hypothesis, (n_reads, n_best, T, N), zeros and logp NaN where i >= n_hyp[r]: ctc_occupancy_batch_raw on this
        result's own arrays.  Arguments as ctc_posterior; wide as ctc_occupancy_batch_raw.  CRF results are refused."""
        return self._lattice("ctc", "occupancy", network_outputs, lengths, band, input_dtype,
                             collapse_repeats=collapse_repeats, wide=wide)

    def crf_score(self, network_outputs, init_states, lengths=None, band=0, input_dtype=None, wide=False):
        """ln P(labelling | posteriors) under the CRF model of every read's result, float64 (n_reads, 1) -- of every
        hypothesis, (n_reads, n_best), NaN where i >= n_hyp[r]: crf_score_batch_raw on this result's own arrays (wide
        included).  For the results of the CRF searches, with the (B,T,S,N) posteriors and init rows they decoded (a
        session: the concatenated posteriors); plain CTC results are refused."""
        return self._lattice("crf", "score", network_outputs, lengths, band, input_dtype, init_states=init_states, wide=wide)

    def crf_align(self, network_outputs, init_states, lengths=None, band=0, input_dtype=None):
        """The best alignment of every read's result under the CRF model -> AlignResult, arrays (n_reads, 1, stride) -- of
        every hypothesis, (n_reads, n_best, stride), logp NaN and count 0 where i >= n_hyp[r]: crf_align_batch_raw on this
        result's own arrays.  Arguments as crf_score."""
        return self._lattice("crf", "align", network_outputs, lengths, band, input_dtype, init_states=init_states)

    def crf_posterior(self, network_outputs, init_states, lengths=None, band=0, input_dtype=None):
        """The substitution posteriors under the CRF model of every read's result -> PosteriorResult, post
        (n_reads, 1, stride, N-1) -- of every hypothesis, (n_reads, n_best, stride, N-1), logp NaN where i >= n_hyp[r]:
        crf_posterior_batch_raw on this result's own arrays.  Arguments as crf_score."""
        return self._lattice("crf", "posterior", network_outputs, lengths, band, input_dtype, init_states=init_states)

    def crf_edits(self, network_outputs, init_states, lengths=None, band=0, input_dtype=None):
        """The deletion and insertion likelihoods under the CRF model of every read's result -> EditResult, deletion
        (n_reads, 1, stride), insertion (n_reads, 1, stride + 1, N-1) -- of every hypothesis, (n_reads, n_best, stride) and
        (n_reads, n_best, stride + 1, N-1), logp NaN where i >= n_hyp[r]: crf_edits_batch_raw on this result's own arrays.
        Arguments as crf_score."""
        return self._lattice("crf", "edits", network_outputs, lengths, band, input_dtype, init_states=init_states)

    def crf_occupancy(self, network_outputs, init_states, lengths=None, band=0, input_dtype=None, wide=False):
        """The edge occupancies under the CRF model of every read's result -> OccupancyResult, occupancy
        (n_reads, 1, T, S, N) -- of every hypothesis, (n_reads, n_best, T, S, N), zeros and logp NaN where i >= n_hyp[r]:
        crf_occupancy_batch_raw on this result's own arrays.  Arguments as crf_score; wide as crf_occupancy_batch_raw."""
        return self._lattice("crf", "occupancy", network_outputs, lengths, band, input_dtype, init_states=init_states,
                             wide=wide)


class BatchResult(_LatticeMethods):
    """Raw outcome of a batched search: label indices, paths, lengths and per-read status.
    Arrays are numpy for host inputs, torch tensors (same device) for device inputs."""

    def __init__(self, labels, path, out_len, status, qual=None, ambiguous=None):
        self.labels, self.path, self.out_len, self.status, self.qual = labels, path, out_len, status, qual
        # beam searches with count_ambiguous=True: (n_reads, 2) tie counters per read -- [:, 0] steps with
        # > 20 candidates and an exact tie involving a kept one, [:, 1] steps with an exact tie at ranks
        # 0 / 1 or across the truncation boundary (include/fcd.h, fcd_result.ambiguous)
        self.ambiguous = ambiguous

    def cpu(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.overlap and not isinstance(self.labels, np.ndarray):
            # the search may have run on one of the handle's internal streams (Handle.set_overlap): the copies below
            # are issued on torch's current stream, which waits for every overlapping call first
            import torch
            h.set_stream(torch.cuda.current_stream(self.labels.device).cuda_stream)
            h.overlap_join()
        return BatchResult(*map(_to_host, (self.labels, self.path, self.out_len, self.status, self.qual, self.ambiguous)))

    def _lattice_refuses(self, model):
        # (crf_*: the posteriors' rank alone tells -- the CRF beam searches return BatchResults as the plain ones do)
        return model == "ctc" and isinstance(self, _CrfBatchResult)

    def _lattice_n_valid(self, band):
        if band and self.path is None:
            raise ValueError("a band needs the result's path")
        return None

    def sequences(self, alphabet, raise_on_error=True, paths="list"):
        """-> list of (str, path) per read, exactly what the single-read functions return.

        paths="list" (default) gives list[int] like the reference; building millions of Python ints
        dominates large batches (4096 reads x ~2000 labels: ~150 ms against a 5 ms kernel), so
        paths="array" returns int32 numpy views into the result instead, and paths=None skips them."""
        if paths not in ("list", "array", None):
            raise ValueError("paths must be 'list', 'array' or None")
        r = self.cpu()
        alpha = _seq_to_vec(alphabet)
        ok = np.ones(len(r.out_len), bool) if r.status is None else (np.asarray(r.status) == nat.ST_OK)
        if raise_on_error and not ok.all():
            i = int(np.flatnonzero(~ok)[0])
            raise RuntimeError("read %d: %s" % (i, nat.status_string(int(r.status[i]))))
        lens = np.asarray(r.out_len).astype(np.int64)
        labels = np.asarray(r.labels)
        single = all(len(a) == 1 and ord(a) < 128 for a in alpha)
        if single:
            # one vectorised table lookup for the whole batch, then a slice + decode per read
            lut = np.zeros(256, np.uint8)
            lut[:len(alpha)] = np.frombuffer("".join(alpha).encode("ascii"), np.uint8)
            chars = lut[labels]
        else:
            table = np.array(alpha, dtype=object)
        out = []
        for i in range(len(lens)):
            if not ok[i]:
                out.append(None)
                continue
            n = int(lens[i])
            if single:
                seq = chars[i, :n].tobytes().decode("ascii")
            else:
                seq = "".join(table[labels[i, :n]]) if n else ""
            if r.path is None or paths is None:
                pth = None
            elif paths == "array":
                pth = r.path[i, :n]
            else:
                pth = r.path[i, :n].tolist()
            out.append((seq, pth))
        return out


def _torch_dtype_code(x):
    import torch
    code = {torch.float32: nat.DTYPE_F32, torch.float16: nat.DTYPE_F16, torch.bfloat16: nat.DTYPE_BF16}.get(x.dtype)
    if code is None:
        raise TypeError("device posteriors must be float32, float16 or bfloat16")
    return code


def _torch_call(fn_name, x, crf, lengths, extra_args, want_qual=False, want_path=True,
                need_status=True, handle=None, want_amb=False, tail_args=()):
    import torch

    # half-precision posteriors (what basecaller networks emit) are read as they are: the kernels convert in
    # registers while loading -- exactly, so the result is the reference's on the upcast matrix -- and compute in f32
    dcode = _torch_dtype_code(x)
    dev = x.device.index or 0
    h = handle if handle is not None else nat.default_handle(dev)
    if crf:
        B, T, S, N = x.shape
        st = x.stride()
        b = nat.Batch(x.data_ptr(), B, T, S, N, st[0], st[1], st[2], st[3], None, dcode)
    else:
        B, T, N = x.shape
        st = x.stride()
        b = nat.Batch(x.data_ptr(), B, T, 1, N, st[0], st[1], 0, st[2], None, dcode)
    if lengths is not None:
        lengths = torch.as_tensor(lengths, dtype=torch.int64, device=x.device).contiguous()
        b.lengths = lengths.data_ptr()
    w = max(int(T), 1)
    labels = torch.empty((B, w), dtype=torch.uint8, device=x.device)
    path = torch.empty((B, w), dtype=torch.int32, device=x.device) if want_path else None
    qual = torch.empty((B, w), dtype=torch.float32, device=x.device) if want_qual else None
    # (the beam kernels write out_len and status of EVERY read on every way out -- no fill kernels in front of them, which
    # under Handle.set_overlap would wait for a free wavefront slot behind the internal streams' high-priority launches)
    beam = fn_name in ("fcd_beam_search_dev", "fcd_crf_beam_search_dev", "fcd_crf_beam_search_dev_k")
    meta = (torch.empty if beam else torch.zeros)((2, B), dtype=torch.int32, device=x.device)
    out_len, status = meta[0], meta[1]
    amb = torch.zeros((B, 2), dtype=torch.int32, device=x.device) if want_amb else None
    res = nat.Result(labels.data_ptr(), path.data_ptr() if want_path else None,
                     qual.data_ptr() if want_qual else None, out_len.data_ptr(),
                     status.data_ptr(), w, amb.data_ptr() if want_amb else None)
    h.set_stream(torch.cuda.current_stream(x.device).cuda_stream)
    fn = getattr(h.lib, fn_name)
    h.check(fn(h.ptr, C.byref(b), *extra_args, C.byref(res), *tail_args))
    r = BatchResult(labels, path, out_len, status, qual, amb)
    r._handle = h
    r._keep = (x, lengths)
    h.hold_in_flight(r._keep, labels, path, qual, out_len, status, amb)
    return r


def _stack_host(x, ndim):
    if isinstance(x, np.ndarray):
        a = x
    else:
        a = np.stack([np.asarray(v) for v in x])
    if a.dtype not in (np.float32, np.float16, np.uint16) or a.ndim != ndim:
        raise TypeError("expected a float32 (or float16 / bfloat16-bits uint16) array of rank %d" % ndim)
    return _dense(a)


def _ragged(network_outputs, lengths, ndim):
    """A list/tuple of per-read arrays of different lengths -> (padded batch, lengths).
    Reads are padded with zeros to the longest one; the kernels never look past lengths[i]."""
    if isinstance(network_outputs, (list, tuple)) and len(network_outputs) > 0 and lengths is None \
            and all(isinstance(v, np.ndarray) for v in network_outputs):
        Ts = [v.shape[0] for v in network_outputs]
        if len(set(Ts)) > 1:
            tail = network_outputs[0].shape[1:]
            if any(v.dtype != np.float32 or v.ndim != ndim - 1 or v.shape[1:] != tail for v in network_outputs):
                raise TypeError("expected float32 arrays of rank %d with equal inner shapes" % (ndim - 1))
            out = np.zeros((len(Ts), max(Ts)) + tail, np.float32)
            for i, v in enumerate(network_outputs):
                out[i, :Ts[i]] = v
            return out, np.asarray(Ts, np.int64)
    return network_outputs, lengths


def _host_input(x):
    """What the compiled batch functions take: one ndarray, or a list of per-read ndarrays."""
    if isinstance(x, np.ndarray):
        return x
    return [np.asarray(v) for v in x]


def _device_tensor(x):
    """torch ROCm tensors pass through; any other device array speaking DLPack (e.g. CuPy) is
    wrapped zero-copy.  Host objects return None."""
    if _is_torch_cuda(x):
        return x
    if hasattr(x, "__dlpack__") and not isinstance(x, np.ndarray) and hasattr(x, "__dlpack_device__"):
        try:
            dev_type = int(x.__dlpack_device__()[0])
        except Exception:
            return None
        if dev_type in (2, 10):  # kDLCUDA, kDLROCM
            import torch
            return torch.from_dlpack(x)
    return None


def beam_search_batch_raw(network_outputs, beam_size=5, beam_cut_threshold=0.0,
                          collapse_repeats=True, lengths=None, kernel=nat.KERNEL_AUTO, handle=None,
                          count_ambiguous=False, input_dtype=None):
    """Decode a (B,T,N) batch with search::beam_search semantics; returns a BatchResult.
    `handle` (device tensors only): an explicit fast_ctc_decode_amd._native.Handle -- one per
    concurrent torch stream, since a handle owns the tree-arena workspace its kernels use.
    `count_ambiguous`: also fill BatchResult.ambiguous (instrumented kernels; include/fcd.h)."""
    dev_x = _device_tensor(network_outputs)
    if dev_x is not None:
        network_outputs = dev_x
        return _torch_call("fcd_beam_search_dev", network_outputs, False, lengths,
                           (int(beam_size), float(beam_cut_threshold),
                            int(bool(collapse_repeats)), int(kernel)), handle=handle,
                           want_amb=count_ambiguous)
    network_outputs, lengths = _ragged(network_outputs, lengths, 3)
    x = _stack_host(network_outputs, 3)
    B, T, N = x.shape
    h = nat.default_handle()
    out = _HostOut(B, T, want_amb=count_ambiguous)
    l = _np_lengths(lengths, B)
    b = _host_batch(x, False, l, input_dtype)
    h.check(h.lib.fcd_beam_search_host(h.ptr, C.byref(b), int(beam_size), float(beam_cut_threshold),
                                       int(bool(collapse_repeats)), int(kernel), C.byref(out.res)))
    return BatchResult(out.labels, out.path, out.out_len, out.status, ambiguous=out.ambiguous)


def beam_search_batch(network_outputs, alphabet, beam_size=5, beam_cut_threshold=0.0,
                      collapse_repeats=True, lengths=None, kernel=nat.KERNEL_AUTO, paths="list"):
    """Batched beam_search: element i equals beam_search(network_outputs[i][:lengths[i]], ...).
    paths="array" returns the paths as numpy arrays instead of list[int] (see BatchResult.sequences)."""
    if _device_tensor(network_outputs) is None:  # host input: the compiled layer streams result chunks
        return _compiled().beam_search_batch(_host_input(network_outputs), alphabet, beam_size, beam_cut_threshold,
                                             collapse_repeats, lengths, paths, int(kernel))
    alpha = _seq_to_vec(alphabet)
    _check_beam_args(len(alpha), network_outputs.shape[-1], beam_size, beam_cut_threshold)
    r = beam_search_batch_raw(network_outputs, beam_size, beam_cut_threshold, collapse_repeats,
                              lengths, kernel)
    return r.sequences(alpha, paths=paths)


def viterbi_search_batch_raw(network_outputs, collapse_repeats=True, lengths=None, qual=False, input_dtype=None):
    dev_x = _device_tensor(network_outputs)
    if dev_x is not None:
        return _torch_call("fcd_viterbi_search_dev", dev_x, False, lengths,
                           (int(bool(collapse_repeats)),), want_qual=qual)
    network_outputs, lengths = _ragged(network_outputs, lengths, 3)
    x = _stack_host(network_outputs, 3)
    B, T, N = x.shape
    h = nat.default_handle()
    out = _HostOut(B, T, want_qual=qual)
    l = _np_lengths(lengths, B)
    b = _host_batch(x, False, l, input_dtype)
    h.check(h.lib.fcd_viterbi_search_host(h.ptr, C.byref(b), int(bool(collapse_repeats)),
                                          C.byref(out.res)))
    return BatchResult(out.labels, out.path, out.out_len, out.status, out.qual)


def viterbi_search_batch(network_outputs, alphabet, qstring=False, qscale=1.0, qbias=0.0,
                         collapse_repeats=True, lengths=None, paths="list"):
    if _device_tensor(network_outputs) is None:
        return _compiled().viterbi_search_batch(_host_input(network_outputs), alphabet, bool(qstring), qscale, qbias,
                                                collapse_repeats, lengths, paths)
    alpha = _seq_to_vec(alphabet)
    _check_greedy_alphabet(len(alpha), network_outputs.shape[-1])
    r = viterbi_search_batch_raw(network_outputs, collapse_repeats, lengths, qual=qstring).cpu()
    res = r.sequences(alpha, paths=paths if paths is not None else "array")
    if qstring:
        res = [(s + _qual_chars(r.qual[i, :len(p)], qscale, qbias), p) for i, (s, p) in enumerate(res)]
    return res


def crf_beam_search_batch_raw(network_outputs, init_states, beam_size=5, beam_cut_threshold=0.0,
                              lengths=None, kernel=nat.KERNEL_AUTO, count_ambiguous=False):
    """(B,T,S,N) posteriors + (B,n_init) initial state scores -> BatchResult."""
    if _is_torch_cuda(network_outputs):
        import torch
        init = torch.as_tensor(init_states, dtype=torch.float32,
                               device=network_outputs.device).contiguous()
        r = _torch_call("fcd_crf_beam_search_dev_k", network_outputs, True, lengths,
                        (C.c_void_p(init.data_ptr()), int(init.shape[1]), int(init.shape[1]),
                         int(beam_size), float(beam_cut_threshold), int(kernel)),
                        want_amb=count_ambiguous)
        r._keep = r._keep + (init,)
        return r
    x = _stack_host(network_outputs, 4)
    init = np.ascontiguousarray(np.asarray(init_states, np.float32))
    B, T, S, N = x.shape
    if init.shape[0] != B or init.ndim != 2:
        raise ValueError("init_states must have shape (n_reads, n_init)")
    h = nat.default_handle()
    out = _HostOut(B, T, want_amb=count_ambiguous)
    l = _np_lengths(lengths, B)
    b = _host_batch(x, True, l)
    h.check(h.lib.fcd_crf_beam_search_host_k(h.ptr, C.byref(b), init.ctypes.data, init.shape[1],
                                             init.shape[1], int(beam_size), float(beam_cut_threshold),
                                             int(kernel), C.byref(out.res)))
    return BatchResult(out.labels, out.path, out.out_len, out.status, ambiguous=out.ambiguous)


def crf_beam_search_batch(network_outputs, init_states, alphabet, beam_size=5,
                          beam_cut_threshold=0.0, lengths=None):
    if _device_tensor(network_outputs) is None:
        return _compiled().crf_beam_search_batch(_host_input(network_outputs), np.asarray(init_states, np.float32),
                                                 alphabet, beam_size, beam_cut_threshold, lengths)
    alpha = _seq_to_vec(alphabet)
    _check_greedy_alphabet(len(alpha), network_outputs.shape[-1])
    r = crf_beam_search_batch_raw(network_outputs, init_states, beam_size, beam_cut_threshold,
                                  lengths).cpu()
    out = []
    for i, item in enumerate(r.sequences(alpha)):
        n = int(r.out_len[i])
        labels = r.labels[i, :n]
        out.append(("".join(alpha[l] for l in labels[::-1])[::-1], item[1]))
    return out


# ---------------------------------------------------------------------------------------------
# n best hypotheses of the beam searches (include/fcd.h, fcd_nbest) -- beyond the reference, which
# returns beam[0] only (src/search.rs:165,300)
# ---------------------------------------------------------------------------------------------
def _check_n_best(n_best, beam_size):
    if isinstance(n_best, bool) or not isinstance(n_best, (int, np.integer)):
        raise TypeError("argument 'n_best': expected an integer")
    if n_best < 1 or n_best > beam_size:
        raise ValueError("n_best must be in 1 .. beam_size (%d), got %d" % (beam_size, n_best))
    return int(n_best)


class NBestResult(_LatticeMethods):
    """Raw outcome of an n-best beam search: hypothesis i of read r is labels[r, i, :out_len[r, i]] (path likewise),
    its score score[r, i] = label_prob + gap_prob of beam entry i after the last step -- relative to the best entry,
    not a log-likelihood.  n_hyp[r] hypotheses per read (0 when the read's search failed: status[r] says why).
    Arrays are numpy for host inputs, torch tensors (same device) for device inputs."""

    def __init__(self, labels, path, out_len, score, n_hyp, status, ambiguous=None, crf=False):
        self.labels, self.path, self.out_len, self.score = labels, path, out_len, score
        self.n_hyp, self.status, self.ambiguous = n_hyp, status, ambiguous
        self.crf = crf  # strings follow crf_beam_search's character reversal (src/search.rs:146-156)

    def cpu(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.overlap and not isinstance(self.labels, np.ndarray):
            import torch  # (as BatchResult.cpu: the copies wait for every overlapping call)
            h.set_stream(torch.cuda.current_stream(self.labels.device).cuda_stream)
            h.overlap_join()
        return NBestResult(*map(_to_host, (self.labels, self.path, self.out_len, self.score, self.n_hyp, self.status,
                                           self.ambiguous)), self.crf)

    def _lattice_refuses(self, model):
        return self.crf != (model == "crf")

    def _lattice_n_valid(self, band):
        return self.n_hyp

    def hypotheses(self, alphabet, raise_on_error=True):
        """-> per read, a list of (seq, path, score), best first (None for a failed read when not raise_on_error)."""
        r = self.cpu()
        alpha = _seq_to_vec(alphabet)
        status = np.asarray(r.status)
        if raise_on_error and (status != nat.ST_OK).any():
            i = int(np.flatnonzero(status != nat.ST_OK)[0])
            raise RuntimeError("read %d: %s" % (i, nat.status_string(int(status[i]))))
        out = []
        for i in range(len(status)):
            if status[i] != nat.ST_OK:
                out.append(None)
                continue
            hyps = []
            for j in range(int(r.n_hyp[i])):
                n = int(r.out_len[i, j])
                labels = r.labels[i, j, :n]
                if self.crf:
                    seq = "".join(alpha[l] for l in labels[::-1])[::-1]
                else:
                    seq = "".join(alpha[l] for l in labels)
                pth = r.path[i, j, :n].tolist() if r.path is not None else None
                hyps.append((seq, pth, float(r.score[i, j])))
            out.append(hyps)
        return out


def _nbest_torch(fn_name, x, crf, lengths, extra_args, n_best, handle=None, want_amb=False):
    import torch

    dcode = _torch_dtype_code(x)
    h = handle if handle is not None else nat.default_handle(x.device.index or 0)
    st = x.stride()
    if crf:
        B, T, S, N = x.shape
        b = nat.Batch(x.data_ptr(), B, T, S, N, st[0], st[1], st[2], st[3], None, dcode)
    else:
        B, T, N = x.shape
        b = nat.Batch(x.data_ptr(), B, T, 1, N, st[0], st[1], 0, st[2], None, dcode)
    if lengths is not None:
        lengths = torch.as_tensor(lengths, dtype=torch.int64, device=x.device).contiguous()
        b.lengths = lengths.data_ptr()
    w = max(int(T), 1)
    # (the kernels write every row, score, n_hyp and status: no fill kernels in front of them)
    labels = torch.empty((B, n_best, w), dtype=torch.uint8, device=x.device)
    path = torch.empty((B, n_best, w), dtype=torch.int32, device=x.device)
    out_len = torch.empty((B, n_best), dtype=torch.int32, device=x.device)
    score = torch.empty((B, n_best), dtype=torch.float32, device=x.device)
    meta = torch.empty((2, B), dtype=torch.int32, device=x.device)
    n_hyp, status = meta[0], meta[1]
    amb = torch.zeros((B, 2), dtype=torch.int32, device=x.device) if want_amb else None
    res = nat.Result(labels.data_ptr(), path.data_ptr(), None, out_len.data_ptr(), status.data_ptr(), w,
                     amb.data_ptr() if want_amb else None)
    nb = nat.NBest(n_best, score.data_ptr(), n_hyp.data_ptr())
    h.set_stream(torch.cuda.current_stream(x.device).cuda_stream)
    h.check(getattr(h.lib, fn_name)(h.ptr, C.byref(b), *extra_args, C.byref(nb), C.byref(res)))
    r = NBestResult(labels, path, out_len, score, n_hyp, status, amb, crf)
    r._handle = h
    r._keep = (x, lengths)
    h.hold_in_flight(r._keep, labels, path, out_len, score, meta, amb)
    return r


class _HostNBest:
    def __init__(self, B, T, n_best, want_amb=False):
        w = max(int(T), 1)
        self.labels = np.zeros((B, n_best, w), np.uint8)
        self.path = np.zeros((B, n_best, w), np.uint32)
        self.out_len = np.zeros((B, n_best), np.uint32)
        self.score = np.zeros((B, n_best), np.float32)
        self.n_hyp = np.zeros(B, np.uint32)
        self.status = np.zeros(B, np.int32)
        self.ambiguous = np.zeros((B, 2), np.uint32) if want_amb else None
        self.res = nat.Result(self.labels.ctypes.data, self.path.ctypes.data, None, self.out_len.ctypes.data,
                              self.status.ctypes.data, w, self.ambiguous.ctypes.data if want_amb else None)
        self.nb = nat.NBest(n_best, self.score.ctypes.data, self.n_hyp.ctypes.data)

    def result(self, crf):
        return NBestResult(self.labels, self.path, self.out_len, self.score, self.n_hyp, self.status, self.ambiguous,
                           crf)


def _check_nbest_raw(n_best, beam_size):
    beam_size = _usize(beam_size, "beam_size")
    if beam_size == 0:
        raise ValueError("beam_size cannot be 0")
    return _check_n_best(n_best, beam_size), beam_size


def beam_search_nbest_batch_raw(network_outputs, n_best, beam_size=5, beam_cut_threshold=0.0, collapse_repeats=True,
                                lengths=None, kernel=nat.KERNEL_AUTO, handle=None, count_ambiguous=False,
                                input_dtype=None):
    """beam_search_batch_raw with the n best hypotheses of every read -> NBestResult (labels (B, n_best, T), path,
    out_len (B, n_best), score (B, n_best), n_hyp (B,), status (B,)).  Hypothesis 0 is what beam_search_batch_raw
    returns for the read."""
    n_best, beam_size = _check_nbest_raw(n_best, beam_size)
    args = (beam_size, float(beam_cut_threshold), int(bool(collapse_repeats)), int(kernel))
    dev_x = _device_tensor(network_outputs)
    if dev_x is not None:
        return _nbest_torch("fcd_beam_search_nbest_dev", dev_x, False, lengths, args, n_best, handle=handle,
                            want_amb=count_ambiguous)
    network_outputs, lengths = _ragged(network_outputs, lengths, 3)
    x = _stack_host(network_outputs, 3)
    B, T, N = x.shape
    h = nat.default_handle()
    out = _HostNBest(B, T, n_best, want_amb=count_ambiguous)
    l = _np_lengths(lengths, B)
    b = _host_batch(x, False, l, input_dtype)
    h.check(h.lib.fcd_beam_search_nbest_host(h.ptr, C.byref(b), *args, C.byref(out.nb), C.byref(out.res)))
    return out.result(False)


def crf_beam_search_nbest_batch_raw(network_outputs, init_states, n_best, beam_size=5, beam_cut_threshold=0.0,
                                    lengths=None, kernel=nat.KERNEL_AUTO, handle=None, count_ambiguous=False,
                                    input_dtype=None):
    """crf_beam_search_batch_raw with the n best hypotheses of every read -> NBestResult (see
    beam_search_nbest_batch_raw); strings from .hypotheses() follow crf_beam_search's character reversal."""
    n_best, beam_size = _check_nbest_raw(n_best, beam_size)
    dev_x = _device_tensor(network_outputs)
    if dev_x is not None:
        import torch
        init = torch.as_tensor(init_states, dtype=torch.float32, device=dev_x.device).contiguous()
        if init.ndim != 2 or init.shape[0] != dev_x.shape[0]:
            raise ValueError("init_states must have shape (n_reads, n_init)")
        r = _nbest_torch("fcd_crf_beam_search_nbest_dev", dev_x, True, lengths,
                         (C.c_void_p(init.data_ptr()), int(init.shape[1]), int(init.shape[1]), beam_size,
                          float(beam_cut_threshold), int(kernel)), n_best, handle=handle, want_amb=count_ambiguous)
        r._keep = r._keep + (init,)
        return r
    x = _stack_host(network_outputs, 4)
    init = np.ascontiguousarray(np.asarray(init_states, np.float32))
    B, T, S, N = x.shape
    if init.ndim != 2 or init.shape[0] != B:
        raise ValueError("init_states must have shape (n_reads, n_init)")
    h = nat.default_handle()
    out = _HostNBest(B, T, n_best, want_amb=count_ambiguous)
    l = _np_lengths(lengths, B)
    b = _host_batch(x, True, l, input_dtype)
    h.check(h.lib.fcd_crf_beam_search_nbest_host(h.ptr, C.byref(b), init.ctypes.data, init.shape[1], init.shape[1],
                                                 beam_size, float(beam_cut_threshold), int(kernel), C.byref(out.nb),
                                                 C.byref(out.res)))
    return out.result(True)


def beam_search_nbest(network_output, alphabet, n_best, beam_size=5, beam_cut_threshold=0.0, collapse_repeats=True):
    """beam_search's search, returning its n best hypotheses: a list of (seq, path, score), best first, of length
    min(n_best, final beam length).  Element 0's (seq, path) is beam_search's result.  score = label_prob + gap_prob
    of the beam entry after the last step, relative to the best entry (<= 1 up to rounding; not a log-likelihood)."""
    x = _as_f32(network_output, 2, "network_output")
    alpha = _seq_to_vec(alphabet)
    _check_beam_args(len(alpha), x.shape[1], beam_size, beam_cut_threshold)
    n_best = _check_n_best(n_best, beam_size)
    r = beam_search_nbest_batch_raw(_dense(x)[None], n_best, beam_size, beam_cut_threshold, collapse_repeats)
    _raise_status(int(r.status[0]))
    return r.hypotheses(alpha)[0]


def crf_beam_search_nbest(network_output, init_state, alphabet, n_best, beam_size=5, beam_cut_threshold=0.0):
    """crf_beam_search's search, returning its n best hypotheses as beam_search_nbest does; element 0's (seq, path) is
    crf_beam_search's result."""
    x = _as_f32(network_output, 3, "network_output")
    init = _as_f32(init_state, 1, "init_state")
    beam_size = _usize(beam_size, "beam_size")
    alpha = _seq_to_vec(alphabet)
    _check_greedy_alphabet(len(alpha), x.shape[2])
    if x.size == 0 or init.size == 0:
        raise RuntimeError("network_output/init_state is empty (the reference asserts and aborts here)")
    if beam_size < 1:
        raise RuntimeError(nat.status_string(nat.ST_RAN_OUT_OF_BEAM))  # truncate(0) -> empty beam
    n_best = _check_n_best(n_best, beam_size)
    r = crf_beam_search_nbest_batch_raw(_dense(x)[None], np.ascontiguousarray(init)[None], n_best, beam_size,
                                        beam_cut_threshold)
    _raise_status(int(r.status[0]))
    return r.hypotheses(alpha)[0]


# ---------------------------------------------------------------------------------------------
# CTC forward log-likelihood of given labellings (include/fcd.h, fcd_ctc_score_*)
# ---------------------------------------------------------------------------------------------
def _score_shapes(labels_shape, B):
    if len(labels_shape) == 2:
        n_hyp, stride = 1, labels_shape[1]
    elif len(labels_shape) == 3:
        n_hyp, stride = labels_shape[1], labels_shape[2]
    else:
        raise ValueError("labels must have shape (n_reads, stride) or (n_reads, n_hyp, stride)")
    if labels_shape[0] != B:
        raise ValueError("labels must have one row (or n_hyp rows) per read")
    if n_hyp < 1:
        raise ValueError("n_hyp must be at least 1")
    return int(n_hyp), int(stride)


def _check_band(band, paths):
    if isinstance(band, bool) or not isinstance(band, (int, np.integer)):
        raise TypeError("argument 'band': expected an integer")
    if band < 0:
        raise ValueError("band must be at least 0")
    if band > 0 and paths is None:
        raise ValueError("a band needs paths (the row at which each label was emitted)")
    return int(band)


def _lattice_inputs(network_outputs, labels, label_lengths, lengths, paths, band, n_valid, input_dtype, handle,
                    init_states=None):
    """The argument handling ctc_score_batch_raw, ctc_align_batch_raw and their CRF counterparts share.  -> (handle,
    nat.Batch, nat.Labellings, (B, n_hyp, stride), device or None for numpy input, the arrays the two structs point into);
    init_states given (the CRF calls: (B, T, S, N) posteriors): the init rows (B, n_init) are the last of those arrays."""
    crf = init_states is not None
    nd = 4 if crf else 3
    dev_x = _device_tensor(network_outputs)
    if dev_x is not None:
        import torch
        x = dev_x
        if x.ndim != nd:
            raise ValueError("expected (n_reads, T, S, N) posteriors" if crf else "expected (n_reads, T, N) posteriors")
        B, T, N = x.shape[0], x.shape[1], x.shape[-1]
        dev = x.device
        h = handle if handle is not None else nat.default_handle(dev.index or 0)

        def as_dev(a, dtype):
            if isinstance(a, np.ndarray) and a.dtype == np.uint32:
                a = a.view(np.int32)  # (the same 32 bits: the searches' device results are int32 tensors)
            a = torch.as_tensor(a, device=dev)
            return (a if a.dtype == dtype else a.to(dtype)).contiguous()
        lab = as_dev(labels, torch.uint8)
        n_hyp, stride = _score_shapes(tuple(lab.shape), B)
        ylen = as_dev(label_lengths, torch.int32)
        if ylen.numel() != B * n_hyp:
            raise ValueError("label_lengths must have one entry per labelling")
        pth = as_dev(paths, torch.int32) if band else None
        if pth is not None and tuple(pth.shape) != tuple(lab.shape):
            raise ValueError("paths must have the shape of labels")
        nv = as_dev(n_valid, torch.int32) if n_valid is not None else None
        if nv is not None and nv.numel() != B:
            raise ValueError("n_valid must have shape (n_reads,)")
        st = x.stride()
        init = None
        if crf:
            init = torch.as_tensor(init_states, dtype=torch.float32, device=dev).contiguous()
            if init.ndim != 2 or init.shape[0] != B or init.shape[1] < 1:
                raise ValueError("init_states must have shape (n_reads, n_init)")
            b = nat.Batch(x.data_ptr(), B, T, x.shape[2], N, st[0], st[1], st[2], st[3], None, _torch_dtype_code(x))
        else:
            b = nat.Batch(x.data_ptr(), B, T, 1, N, st[0], st[1], 0, st[2], None, _torch_dtype_code(x))
        if lengths is not None:
            lengths = torch.as_tensor(lengths, dtype=torch.int64, device=dev).contiguous()
            if lengths.numel() != B:
                raise ValueError("lengths must have shape (n_reads,)")
            b.lengths = lengths.data_ptr()
        y = nat.Labellings(lab.data_ptr(), ylen.data_ptr(), nv.data_ptr() if nv is not None else None,
                           pth.data_ptr() if pth is not None else None, n_hyp, stride)
        h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        return h, b, y, (B, n_hyp, stride), dev, (x, lab, ylen, pth, nv, lengths, init)
    network_outputs, lengths = _ragged(network_outputs, lengths, nd)
    x = _stack_host(network_outputs, nd)
    B, T, N = x.shape[0], x.shape[1], x.shape[-1]
    lab = np.ascontiguousarray(np.asarray(labels), np.uint8)
    n_hyp, stride = _score_shapes(lab.shape, B)
    ylen = np.ascontiguousarray(np.asarray(label_lengths), np.uint32)
    if ylen.size != B * n_hyp:
        raise ValueError("label_lengths must have one entry per labelling")
    pth = np.ascontiguousarray(np.asarray(paths), np.uint32) if band else None
    if pth is not None and pth.shape != lab.shape:
        raise ValueError("paths must have the shape of labels")
    nv = np.ascontiguousarray(np.asarray(n_valid), np.uint32) if n_valid is not None else None
    if nv is not None and nv.shape != (B,):
        raise ValueError("n_valid must have shape (n_reads,)")
    h = nat.default_handle()  # (host arrays: the calling thread's own handle, whatever handle the search ran on)
    l = _np_lengths(lengths, B)
    init = None
    if crf:
        init = np.ascontiguousarray(np.asarray(init_states, np.float32))
        if init.ndim != 2 or init.shape[0] != B or init.shape[1] < 1:
            raise ValueError("init_states must have shape (n_reads, n_init)")
    b = _host_batch(x, crf, l, input_dtype)
    y = nat.Labellings(lab.ctypes.data, ylen.ctypes.data, nv.ctypes.data if nv is not None else None,
                       pth.ctypes.data if pth is not None else None, n_hyp, stride)
    return h, b, y, (B, n_hyp, stride), None, (x, lab, ylen, pth, nv, l, init)


class _Arrays:
    """Where a lattice call's outputs live: torch tensors on `dev`, numpy arrays for dev=None.  zeros / empty(shape, kind)
    with kind u32 (an int32 tensor on the device: the same 32 bits), f32 or f64; ptr(a): the address the C ABI takes."""

    def __init__(self, dev):
        self.dev = dev

    def _new(self, how, shape, kind):
        if self.dev is None:
            return getattr(np, how)(shape, {"u32": np.uint32, "f32": np.float32, "f64": np.float64}[kind])
        import torch
        dtype = {"u32": torch.int32, "f32": torch.float32, "f64": torch.float64}[kind]
        return getattr(torch, how)(shape, dtype=dtype, device=self.dev)

    def zeros(self, shape, kind):
        return self._new("zeros", shape, kind)

    def empty(self, shape, kind):
        return self._new("empty", shape, kind)

    def ptr(self, a):
        return a.ctypes.data if self.dev is None else a.data_ptr()


# The outputs of each kind of lattice call: (xp, the call's nat.Batch, (B, n_hyp, stride)) -> (the C ABI's last argument,
# what the Python call returns).  logp and the scores are written for every labelling (empty), the rest only where there is
# something to say (zeros).
def _score_out(xp, b, shape):
    out = xp.empty(shape[:2], "f64")
    return C.c_void_p(xp.ptr(out)), out


def _align_out(xp, b, shape):
    start, count, qual = xp.zeros(shape, "u32"), xp.zeros(shape, "u32"), xp.zeros(shape, "f32")
    logp = xp.empty(shape[:2], "f64")
    out = nat.Alignment(xp.ptr(start), xp.ptr(count), xp.ptr(qual), xp.ptr(logp))
    return C.byref(out), AlignResult(start, count, qual, logp)


def _posterior_out(xp, b, shape):
    post = xp.zeros(shape + (int(b.N) - 1,), "f32")
    logp = xp.empty(shape[:2], "f64")
    return C.byref(nat.Posterior(xp.ptr(post), xp.ptr(logp))), PosteriorResult(post, logp)


def _edits_out(xp, b, shape):
    B, n_hyp, stride = shape
    dele = xp.zeros(shape, "f32")
    ins = xp.zeros((B, n_hyp, stride + 1, int(b.N) - 1), "f32")
    logp = xp.empty(shape[:2], "f64")
    return C.byref(nat.Edits(xp.ptr(dele), xp.ptr(ins), xp.ptr(logp))), EditResult(dele, ins, logp)


def _occupancy_block(out_shape, shape5, elem_strides):
    """the caller's buffer as fcd_occupancy sees it -> (stride_row, stride_t); shape5 = (B, n_hyp, T, S, N)"""
    B, n_hyp, T, S, N = shape5
    if tuple(out_shape) == (B, T, S, N) and n_hyp == 1:
        st = (elem_strides[0], elem_strides[0]) + tuple(elem_strides[1:])
    elif tuple(out_shape) == shape5:
        st = tuple(elem_strides)
    else:
        raise ValueError("out must have shape (n_reads, n_hyp, T, S, N) (or (n_reads, T, S, N) for one labelling per read)")
    if B * n_hyp * T == 0:
        return S * N, S * N
    if (N > 1 and st[4] != 1) or (S > 1 and st[3] != N):
        raise ValueError("out: the (S, N) rows must be dense")
    if any(v < 0 for v in st) or (T > 1 and st[2] < S * N) or (n_hyp > 1 and B > 1 and st[0] != n_hyp * st[1]):
        raise ValueError("out: labelling blocks must be evenly spaced, rows at least S * N floats apart")
    return (st[1] if n_hyp > 1 or B == 1 else st[0]), max(st[2], S * N)


def _check_occupancy_out(out=None, scale=1.0, accumulate=False, time_major_out=False):
    """what the occupancy calls refuse before they look at their inputs (arguments: _occupancy_out's)"""
    if accumulate and out is None:
        raise ValueError("accumulate=True needs the buffer to add to: pass out")
    if out is not None and time_major_out:
        raise ValueError("time_major_out shapes the array the call allocates: pass either out or time_major_out")


def _occupancy_out(xp, b, shape, has_S, out=None, scale=1.0, accumulate=False, time_major_out=False):
    """has_S: (B, n_hyp, T, S, N) occupancies of a CRF model; else (B, n_hyp, T, N), which fcd_occupancy takes as S = 1 --
    its (S, N) row is the row of N"""
    B, n_hyp = shape[:2]
    T, S, N = int(b.T), int(b.S), int(b.N)
    cell = (S, N) if has_S else (N,)
    if out is None:
        occ = xp.zeros(((T, B, n_hyp) if time_major_out else (B, n_hyp, T)) + cell, "f32")
        if time_major_out:
            order = (1, 2, 0) + tuple(range(3, occ.ndim))
            occ = occ.transpose(order) if xp.dev is None else occ.permute(order)
    elif xp.dev is not None:
        import torch
        if not _is_torch_cuda(out) or out.device != xp.dev or out.dtype != torch.float32:
            raise TypeError("out must be a float32 tensor on the inputs' device")
        occ = out
    else:
        if not isinstance(out, np.ndarray) or out.dtype != np.float32 or not out.flags.writeable:
            raise TypeError("out must be a writable float32 numpy array")
        occ = out
    shp = tuple(occ.shape)
    st = tuple(v // 4 for v in occ.strides) if xp.dev is None else tuple(occ.stride())  # (in elements)
    if not has_S:
        if occ.ndim not in (3, 4):
            raise ValueError("out must have shape (n_reads, n_hyp, T, N) (or (n_reads, T, N) for one labelling per read)")
        shp, st = shp[:-1] + (1, shp[-1]), st[:-1] + (N, st[-1])
    sr, stt = _occupancy_block(shp, (B, n_hyp, T, S, N), st)
    logp = xp.empty((B, n_hyp), "f64")
    o = nat.Occupancy(xp.ptr(occ), sr, stt, float(scale), int(bool(accumulate)), xp.ptr(logp))
    return C.byref(o), OccupancyResult(occ, logp)


_LATTICE_BUILDERS = {"score": _score_out, "align": _align_out, "posterior": _posterior_out, "edits": _edits_out,
                     "occupancy": _occupancy_out}


@contextlib.contextmanager
def _wide_switch(h, model, wide):
    """The handle's wide switch of `model` (include/fcd.h: fcd_set_ctc_occupancy_wide, fcd_set_crf_lattice_wide) on around
    one call and off behind it, whatever the call raised; nothing where wide is false.  The handle is this thread's:
    nothing else calls between the switch and the call."""
    if not wide:
        yield
        return
    switch = h.set_crf_lattice_wide if model == "crf" else h.set_ctc_occupancy_wide
    switch(True)
    try:
        yield
    finally:
        switch(False)


def _lattice_call(model, kind, network_outputs, labels, label_lengths, lengths, paths, band, n_valid, input_dtype, handle,
                  init_states=None, collapse_repeats=True, wide=False, **out_args):
    """The one body of the ten labelling-lattice calls: fcd_<model>_<kind>_dev for device tensors, _host for numpy, with
    model "ctc" (network_outputs (B,T,N), collapse_repeats) or "crf" ((B,T,S,N) and init_states), kind one of
    _LATTICE_BUILDERS; out_args: the occupancy calls' out, scale, accumulate and time_major_out.  -> what the call returns."""
    band = _check_band(band, paths)
    if kind == "occupancy":
        _check_occupancy_out(**out_args)
        out_args["has_S"] = model == "crf"
    h, b, y, shape, dev, keep = _lattice_inputs(network_outputs, labels, label_lengths, lengths, paths, band, n_valid,
                                                input_dtype, handle, init_states)
    xp = _Arrays(dev)
    out, result = _LATTICE_BUILDERS[kind](xp, b, shape, **out_args)
    if model == "crf":
        init = keep[-1]
        args = (C.byref(b), C.c_void_p(xp.ptr(init)), int(init.shape[1]), int(init.shape[1]), C.byref(y), band, out)
    else:
        args = (C.byref(b), C.byref(y), int(bool(collapse_repeats)), band, out)
    fn = getattr(h.lib, "fcd_%s_%s_%s" % (model, kind, "host" if dev is None else "dev"))
    with _wide_switch(h, model, wide):
        h.check(fn(h.ptr, *args))
    if kind == "occupancy" and dev is not None:
        h.hold_in_flight(result.occupancy, result.logp, *keep)
    return result


def ctc_score_batch_raw(network_outputs, labels, label_lengths, collapse_repeats=True, lengths=None, paths=None,
                        band=0, n_valid=None, input_dtype=None, handle=None):
    """CTC forward log-likelihood ln P(y | x) of labellings y against the (B,T,N) posteriors x: the sum over every
    alignment, not the beam search's pruned estimate -- float64, comparable between reads (include/fcd.h,
    fcd_ctc_score_*).  -> (B, n_hyp) float64.

    labels (B, stride) or (B, n_hyp, stride) uint8 label indices 1 .. N-1 and label_lengths (B,) / (B, n_hyp), as the
    searches return them (BatchResult / NBestResult: .labels, .out_len).  band=0 scores the exact lattice; band=W > 0
    only the alignments within W labels of `paths` (same shape as labels: the row each label was emitted at) -- a
    lower bound that rises with W, at a cost that no longer grows with the labelling's length.  n_valid (B,): rows
    i >= n_valid[r] are not scored (NaN).  Device tensors in: a torch tensor on the same device, enqueued on torch's
    current stream, not synchronised.  numpy in: numpy out."""
    return _lattice_call("ctc", "score", network_outputs, labels, label_lengths, lengths, paths, band, n_valid, input_dtype,
                         handle, collapse_repeats=collapse_repeats)


def _sequence_labels(sequence, alpha, what):
    if not isinstance(sequence, str):
        raise TypeError("argument 'sequence': expected str")
    if any(len(a) != 1 for a in alpha[1:]):
        raise ValueError("%s needs single-character labels" % what)
    index = {a: i for i, a in enumerate(alpha) if i > 0}
    try:
        return [index[c] for c in sequence]
    except KeyError as e:
        raise ValueError("sequence holds %r, which is not a label of the alphabet" % e.args[0])


def _ctc_one_read(network_output, sequence, alphabet, what):
    """One (T, N) matrix and one string as the batch calls take them -> (x (1, T, N), labels (1, max(L, 1)), lengths (1,), L)"""
    x = _as_f32(network_output, 2, "network_output")
    alpha = _seq_to_vec(alphabet)
    _check_greedy_alphabet(len(alpha), x.shape[1])
    y = _sequence_labels(sequence, alpha, what)
    lab = np.zeros((1, max(len(y), 1)), np.uint8)
    lab[0, :len(y)] = y
    return _dense(x)[None], lab, np.array([len(y)], np.uint32), len(y)


def ctc_score(network_output, sequence, alphabet, collapse_repeats=True):
    """ln P(sequence | network_output): the CTC forward log-likelihood of one string against one (T, N) float32
    posterior matrix, exact (every alignment), as a float.  alphabet[0] is the blank; every label must be one
    character (a multi-character alphabet cannot be split back unambiguously: ValueError)."""
    x, lab, n, _ = _ctc_one_read(network_output, sequence, alphabet, "ctc_score")
    return float(ctc_score_batch_raw(x, lab, n, collapse_repeats)[0, 0])


# ---------------------------------------------------------------------------------------------
# CTC forced alignment of given labellings (include/fcd.h, fcd_ctc_align_*)
# ---------------------------------------------------------------------------------------------
class AlignResult:
    """Outcome of ctc_align_batch_raw: for label k of hypothesis i of read r, start[r, i, k] is the first row the best
    alignment spends in it, count[r, i, k] how many (consecutive) rows, qual[r, i, k] the mean posterior of the label
    over them (float32: what viterbi_search turns into its quality string); logp[r, i] (float64) is ln of the
    alignment's probability -- NaN / -inf where there is none, and count is 0 there (include/fcd.h).  Entries
    k >= the labelling's length are 0.  numpy for host inputs, torch tensors (same device) for device inputs."""

    def __init__(self, start, count, qual, logp):
        self.start, self.count, self.qual, self.logp = start, count, qual, logp

    def cpu(self):
        start, count = _to_host(self.start), _to_host(self.count)
        if start.dtype != np.uint32:  # (device results are int32 tensors: the same 32 bits)
            start, count = start.view(np.uint32), count.view(np.uint32)
        return AlignResult(start, count, _to_host(self.qual), _to_host(self.logp))

    def qstrings(self, out_len, qscale=1.0, qbias=0.0):
        """-> per read, per hypothesis, the phred quality string of its first out_len[r, i] labels (fcd_phred: the
        reference's phred(), src/search.rs:21-36); "" for a labelling without an alignment."""
        r = self.cpu()
        n = np.asarray(_to_host(out_len)).reshape(r.logp.shape)
        return [[_qual_chars(r.qual[b, i, :int(n[b, i])], qscale, qbias) if np.isfinite(r.logp[b, i]) else ""
                 for i in range(r.logp.shape[1])] for b in range(r.logp.shape[0])]


def ctc_align_batch_raw(network_outputs, labels, label_lengths, collapse_repeats=True, lengths=None, paths=None,
                        band=0, n_valid=None, input_dtype=None, handle=None):
    """CTC forced alignment: the best single alignment of every labelling to its read's rows -- which rows belong to each
    label, the label's quality as viterbi_search defines it, and ln of the alignment's probability (include/fcd.h,
    fcd_ctc_align_*).  -> AlignResult with start, count, qual (B, n_hyp, stride) and logp (B, n_hyp).

    Arguments as ctc_score_batch_raw: band=0 aligns in the exact lattice, band=W > 0 within W labels of `paths`.
    Device tensors in: torch tensors on the same device, enqueued on torch's current stream, not synchronised.
    numpy in: numpy out."""
    return _lattice_call("ctc", "align", network_outputs, labels, label_lengths, lengths, paths, band, n_valid, input_dtype,
                         handle, collapse_repeats=collapse_repeats)


def ctc_align(network_output, sequence, alphabet, collapse_repeats=True):
    """The best alignment of one string to one (T, N) float32 posterior matrix, exact lattice: -> (spans, quals, logp)
    with spans = [(start, count)] per character, quals = the mean posterior of each over its rows, logp = ln of the
    alignment's probability.  No alignment (more characters than rows, ...): ([], [], -inf)."""
    x, lab, n, L = _ctc_one_read(network_output, sequence, alphabet, "ctc_align")
    r = ctc_align_batch_raw(x, lab, n, collapse_repeats)
    logp = float(r.logp[0, 0])
    if not np.isfinite(logp):
        return [], [], logp
    return ([(int(s), int(c)) for s, c in zip(r.start[0, 0, :L], r.count[0, 0, :L])],
            [float(q) for q in r.qual[0, 0, :L]], logp)


# ---------------------------------------------------------------------------------------------
# CTC forward-backward substitution posteriors of given labellings (include/fcd.h, fcd_ctc_posterior_*)
# ---------------------------------------------------------------------------------------------
class PosteriorResult:
    """Outcome of ctc_posterior_batch_raw and crf_posterior_batch_raw: post[r, i, k, c - 1] is the posterior that label c stands at position k of
    hypothesis i of read r, the rest of the labelling held fixed -- P(y[k:=c] | x) over its sum over c, float32, all
    alignments counted (include/fcd.h); logp[r, i] (float64) is ln P(y | x), ctc_score's (crf_score's) value.  NaN for every position of
    a labelling whose P is not positive and finite; entries k >= the labelling's length are 0.  numpy for host inputs,
    torch tensors (same device) for device inputs."""

    def __init__(self, post, logp):
        self.post, self.logp = post, logp

    def cpu(self):
        return PosteriorResult(_to_host(self.post), _to_host(self.logp))

    def conf(self, labels):
        """-> (B, n_hyp, stride) float32 numpy: the called label's share, post[r, i, k, labels[r, i, k] - 1]; 0 where the
        entry of `labels` is no label (the padding behind a labelling)."""
        post = self.cpu().post
        lab = np.asarray(_to_host(labels)).astype(np.int64).reshape(post.shape[:3])
        ok = (lab >= 1) & (lab <= post.shape[3])
        col = np.where(ok, lab - 1, 0)
        return np.where(ok, np.take_along_axis(post, col[..., None], 3)[..., 0], np.float32(0.0)).astype(np.float32)

    def qstrings(self, labels, out_len, qscale=1.0, qbias=0.0):
        """-> per read, per hypothesis, the phred quality string of its first out_len[r, i] labels, from conf through the
        conversion AlignResult.qstrings uses (fcd_phred); "" for a labelling without a posterior."""
        logp = self.cpu().logp
        conf = self.conf(labels)
        n = np.asarray(_to_host(out_len)).reshape(logp.shape)
        return [[_qual_chars(conf[b, i, :int(n[b, i])], qscale, qbias) if np.isfinite(logp[b, i]) else ""
                 for i in range(logp.shape[1])] for b in range(logp.shape[0])]


def ctc_posterior_batch_raw(network_outputs, labels, label_lengths, collapse_repeats=True, lengths=None, paths=None,
                            band=0, n_valid=None, input_dtype=None, handle=None):
    """CTC forward-backward substitution posteriors: for every position of every labelling, the posterior over which
    label stands there with the rest of the labelling held fixed, summed over every alignment in one forward and one
    backward walk (include/fcd.h, fcd_ctc_posterior_*).  -> PosteriorResult with post (B, n_hyp, stride, N-1) float32
    and logp (B, n_hyp) float64.

    Arguments as ctc_score_batch_raw: band=0 walks the exact lattice, band=W > 0 the window within W labels of `paths`.
    Limits: windows of at most 510 states (bands up to 126, exact mode up to 254 rows or labels) and N - 1 <= 8.
    Device tensors in: torch tensors on the same device, enqueued on torch's current stream, not synchronised.
    numpy in: numpy out."""
    return _lattice_call("ctc", "posterior", network_outputs, labels, label_lengths, lengths, paths, band, n_valid,
                         input_dtype, handle, collapse_repeats=collapse_repeats)


def ctc_posterior(network_output, sequence, alphabet, collapse_repeats=True):
    """The substitution posteriors of one string against one (T, N) float32 posterior matrix, exact lattice:
    -> (post, logp) with post an (L, N-1) float32 array (row k: the posterior over alphabet[1:] at character k) and
    logp = ln P(sequence | network_output).  Argument checks as ctc_score."""
    x, lab, n, L = _ctc_one_read(network_output, sequence, alphabet, "ctc_posterior")
    r = ctc_posterior_batch_raw(x, lab, n, collapse_repeats)
    return r.post[0, 0, :L].copy(), float(r.logp[0, 0])


# ---------------------------------------------------------------------------------------------
# CTC deletion and insertion likelihoods of given labellings (include/fcd.h, fcd_ctc_edits_*)
# ---------------------------------------------------------------------------------------------
EDIT_NONE, EDIT_DELETION, EDIT_INSERTION, EDIT_SUBSTITUTION = 0, 1, 2, 3


class EditResult:
    """Outcome of ctc_edits_batch_raw and crf_edits_batch_raw, float32 log-ratios against the labelling itself (include/fcd.h): deletion[r, i, k] =
    ln P(y without label k | x) - ln P(y | x) and insertion[r, i, g, c - 1] = ln P(y with label c inserted before label g,
    g = L: at the end | x) - ln P(y | x) for hypothesis i of read r, all alignments counted -- a positive entry is an edit
    that explains the read better than y.  logp[r, i] (float64) is ln P(y | x), ctc_score's value.  -inf: a variant without
    an alignment; NaN for every entry of a labelling whose P is not positive and finite; entries beyond the labelling are
    0.  numpy for host inputs, torch tensors (same device) for device inputs."""

    def __init__(self, deletion, insertion, logp):
        self.deletion, self.insertion, self.logp = deletion, insertion, logp

    def cpu(self):
        return EditResult(_to_host(self.deletion), _to_host(self.insertion), _to_host(self.logp))

    def best(self, out_len, posterior=None, labels=None):
        """The best single edit of every labelling -> (kind, position, label, log_ratio), numpy arrays of shape
        (n_reads, n_hyp): kind EDIT_NONE / EDIT_DELETION (of label `position`) / EDIT_INSERTION (of `label` before label
        `position`) / EDIT_SUBSTITUTION (of label `position` by `label`), label 0 for a deletion, log_ratio float64.
        With a PosteriorResult of the same labellings and their `labels`, substitutions take part: their log-ratio is
        ln(post[k][c] / post[k][y_k]).  EDIT_NONE with 0.0 when no edit has a positive log-ratio; NaN entries take no
        part; among equal ones the first in the order deletions, insertions, substitutions, each by position, then
        label."""
        r = self.cpu()
        B, H, S = r.deletion.shape
        nc = r.insertion.shape[3]
        n = np.asarray(_to_host(out_len)).astype(np.int64).reshape(B, H)
        with np.errstate(all="ignore"):
            d = np.where((np.arange(S) < n[..., None]) & ~np.isnan(r.deletion), r.deletion.astype(np.float64), -np.inf)
            ok = (np.arange(S + 1) <= n[..., None])[..., None] & ~np.isnan(r.insertion)
            parts = [d, np.where(ok, r.insertion.astype(np.float64), -np.inf).reshape(B, H, -1)]
            if posterior is not None:
                if labels is None:
                    raise ValueError("substitutions need the labels next to the PosteriorResult")
                post = posterior.cpu().post.astype(np.float64)
                lab = np.asarray(_to_host(labels)).astype(np.int64).reshape(B, H, S)
                own = (lab >= 1) & (lab <= nc) & (np.arange(S) < n[..., None])
                conf = np.take_along_axis(post, np.where(own, lab - 1, 0)[..., None], 3)
                sub = np.log(post) - np.log(conf)
                keep = own[..., None] & (np.arange(nc) != (lab - 1)[..., None]) & ~np.isnan(sub)
                parts.append(np.where(keep, sub, -np.inf).reshape(B, H, -1))
        every = np.concatenate(parts, 2)
        idx = every.argmax(2) if every.shape[2] else np.zeros((B, H), np.int64)
        val = np.take_along_axis(every, idx[..., None], 2)[..., 0] if every.shape[2] else np.full((B, H), -np.inf)
        n_ins = (S + 1) * nc
        kind = np.where(idx < S, EDIT_DELETION, np.where(idx < S + n_ins, EDIT_INSERTION, EDIT_SUBSTITUTION))
        rest = np.where(kind == EDIT_INSERTION, idx - S, idx - S - n_ins)
        pos = np.where(kind == EDIT_DELETION, idx, rest // max(nc, 1))
        lab_out = np.where(kind == EDIT_DELETION, 0, rest % max(nc, 1) + 1)
        none = ~(val > 0.0)
        return (np.where(none, EDIT_NONE, kind).astype(np.int32), np.where(none, 0, pos).astype(np.int32),
                np.where(none, 0, lab_out).astype(np.int32), np.where(none, 0.0, val))


def ctc_edits_batch_raw(network_outputs, labels, label_lengths, collapse_repeats=True, lengths=None, paths=None,
                        band=0, n_valid=None, input_dtype=None, handle=None):
    """CTC deletion and insertion likelihoods: for every label of every labelling how much better or worse the read is
    explained without it, and for every gap and every label how much better or worse with that label inserted there, as
    log-ratios against the labelling itself, summed over every alignment in one forward and one backward walk
    (include/fcd.h, fcd_ctc_edits_*).  With ctc_posterior_batch_raw's substitutions: every labelling one edit away.
    -> EditResult with deletion (B, n_hyp, stride), insertion (B, n_hyp, stride + 1, N-1) float32 and logp (B, n_hyp)
    float64.

    Arguments as ctc_score_batch_raw: band=0 walks the exact lattice, band=W > 0 the window within W labels of `paths`.
    Limits: windows of at most 510 states (bands up to 126, exact mode up to 254 rows or labels) and N - 1 <= 8.
    Device tensors in: torch tensors on the same device, enqueued on torch's current stream, not synchronised.
    numpy in: numpy out."""
    return _lattice_call("ctc", "edits", network_outputs, labels, label_lengths, lengths, paths, band, n_valid, input_dtype,
                         handle, collapse_repeats=collapse_repeats)


def ctc_edits(network_output, sequence, alphabet, collapse_repeats=True):
    """The deletion and insertion likelihoods of one string against one (T, N) float32 posterior matrix, exact lattice:
    -> (deletion, insertion, logp) with deletion an (L,) and insertion an (L + 1, N-1) float32 array of log-ratios
    (insertion[g, c - 1]: alphabet[c] inserted before character g) and logp = ln P(sequence | network_output).  Argument
    checks as ctc_score."""
    x, lab, n, L = _ctc_one_read(network_output, sequence, alphabet, "ctc_edits")
    r = ctc_edits_batch_raw(x, lab, n, collapse_repeats)
    return r.deletion[0, 0, :L].copy(), r.insertion[0, 0, :L + 1].copy(), float(r.logp[0, 0])


# ---------------------------------------------------------------------------------------------
# CRF scoring and forced alignment of given labellings (include/fcd.h, fcd_crf_score_* / fcd_crf_align_*)
# ---------------------------------------------------------------------------------------------
def crf_score_batch_raw(network_outputs, init_states, labels, label_lengths, lengths=None, paths=None, band=0,
                        n_valid=None, input_dtype=None, handle=None, wide=False):
    """ln of the sum, over every alignment of labelling y to the rows of its read, of the product of the (B,T,S,N) CRF
    posteriors along it, the model state following the labelling from the init row's first maximum as crf_beam_search's
    does (include/fcd.h, fcd_crf_score_*).  -> (B, n_hyp) float64, comparable between the hypotheses of a read and
    between reads.

    labels / label_lengths / paths / band / n_valid as ctc_score_batch_raw; init_states (B, n_init).  band=0 scores the
    whole lattice (labellings up to 511 labels), band=W > 0 the alignments within W labels of `paths` (W <= 255).
    wide=True lifts both (include/fcd.h, fcd_set_crf_lattice_wide): windows up to 4096 states -- 4095 rows or labels, bands
    up to 2047 -- at N - 1 <= 8, walked in LDS beyond 512 states; a window within 512 states runs the same launch and
    returns the same bits as wide=False.
    Device tensors in: a torch tensor on the same device, enqueued on torch's current stream, not synchronised.
    numpy in: numpy out."""
    return _lattice_call("crf", "score", network_outputs, labels, label_lengths, lengths, paths, band, n_valid, input_dtype,
                         handle, init_states, wide=wide)


def crf_align_batch_raw(network_outputs, init_states, labels, label_lengths, lengths=None, paths=None, band=0,
                        n_valid=None, input_dtype=None, handle=None):
    """The best single alignment of every labelling under the CRF model: the row each label is emitted at (start; count
    is 1), the posterior of that emission (qual: what crf_greedy_search turns into its quality string) and ln of the
    alignment's probability (include/fcd.h, fcd_crf_align_*).  -> AlignResult, arrays (B, n_hyp, stride) and logp
    (B, n_hyp).  Arguments as crf_score_batch_raw."""
    return _lattice_call("crf", "align", network_outputs, labels, label_lengths, lengths, paths, band, n_valid, input_dtype,
                         handle, init_states)


def crf_posterior_batch_raw(network_outputs, init_states, labels, label_lengths, lengths=None, paths=None, band=0,
                            n_valid=None, input_dtype=None, handle=None):
    """Forward-backward substitution posteriors under the CRF model: for every position of every labelling, the posterior
    over which label stands there with the rest of the labelling held fixed -- each variant with its own model-state
    trajectory -- summed over every alignment in one forward and one backward walk (include/fcd.h, fcd_crf_posterior_*).
    -> PosteriorResult with post (B, n_hyp, stride, N-1) float32 and logp (B, n_hyp) float64, crf_score's value.

    Arguments as crf_score_batch_raw.  Limits: S = (N - 1)^m and N - 1 <= 8; windows of up to 512 states where
    m (N - 1) <= 8 (S = 4, 16 at N = 5; 256 states where N - 1 > 4), up to 192 states (band <= 95) where m (N - 1) <= 24
    (S = 64, 1024, 4096 at N = 5).
    Device tensors in: torch tensors on the same device, enqueued on torch's current stream, not synchronised.
    numpy in: numpy out."""
    return _lattice_call("crf", "posterior", network_outputs, labels, label_lengths, lengths, paths, band, n_valid,
                         input_dtype, handle, init_states)


def crf_edits_batch_raw(network_outputs, init_states, labels, label_lengths, lengths=None, paths=None, band=0,
                        n_valid=None, input_dtype=None, handle=None):
    """CRF deletion and insertion likelihoods: for every label of every labelling how much better or worse the read is
    explained without it, and for every gap and every label how much better or worse with that label inserted there --
    each variant with its own model-state trajectory -- as log-ratios against the labelling itself, summed over every
    alignment in one forward and two backward walks (include/fcd.h, fcd_crf_edits_*).  With crf_posterior_batch_raw's
    substitutions: every labelling one edit away.
    -> EditResult with deletion (B, n_hyp, stride), insertion (B, n_hyp, stride + 1, N-1) float32 and logp (B, n_hyp)
    float64, crf_score's value within its tolerance.

    Arguments and limits as crf_posterior_batch_raw.
    Device tensors in: torch tensors on the same device, enqueued on torch's current stream, not synchronised.
    numpy in: numpy out."""
    return _lattice_call("crf", "edits", network_outputs, labels, label_lengths, lengths, paths, band, n_valid, input_dtype,
                         handle, init_states)


class OccupancyResult:
    """crf_occupancy_batch_raw's result: occupancy (B, n_hyp, T, S, N) float32 -- scale times the probability, over the
    alignments of labelling (b, i), that the model leaves state s by symbol a at row t (the caller's `out` where one was
    given; a view of a (T, B, n_hyp, S, N) array under time_major_out) -- and logp (B, n_hyp) float64, crf_score's value.
    ctc_occupancy_batch_raw's result: occupancy (B, n_hyp, T, N), the probability that row t emits symbol c, and ctc_score's
    logp.  numpy arrays, or torch tensors on the input's device."""

    def __init__(self, occupancy, logp):
        self.occupancy, self.logp = occupancy, logp

    def cpu(self):
        """-> an OccupancyResult of numpy arrays (device results: waits for them)"""
        if isinstance(self.logp, np.ndarray):
            return self
        return OccupancyResult(self.occupancy.cpu().numpy(), self.logp.cpu().numpy())


def crf_occupancy_batch_raw(network_outputs, init_states, labels, label_lengths, lengths=None, paths=None, band=0,
                            n_valid=None, out=None, scale=1.0, accumulate=False, time_major_out=False, input_dtype=None,
                            handle=None, wide=False):
    """The edge occupancies of every labelling's own lattice under the CRF model: occupancy[b][i][t][s][a] is the
    probability, over the alignments of labelling (b, i) to its read, that the model leaves state s by symbol a at row t
    -- a soft alignment, and the labelled counterpart of crf_marginals_batch_raw's marginals: for raw
    scores x and (network_outputs, init_states) = crf_transition_probs_batch_raw(x), occupancy - marginals is the gradient
    of ln P(labelling, start state | x) (include/fcd.h, fcd_crf_occupancy_*; crf_ctc_loss is that composition).
    -> OccupancyResult with occupancy (B, n_hyp, T, S, N) float32 and logp (B, n_hyp) float64, crf_score's value bit for
    bit.  For every labelling with a finite logp every row t < lengths[b] sums to 1.  The walks keep one float32 exponent
    per row: a long read that does not support its labelling (near-uniform posteriors, many rows per label) is outside what
    they hold; the walk checks every row's sum and gives such a labelling up -- logp NaN and NaN in its rows -- rather than
    return occupancies that do not add up (include/fcd.h has the rule and the measured range).

    Arguments as crf_score_batch_raw; any S it takes, N - 1 <= 8, windows up to 512 states, S * N up to about 39800.
    wide=True lifts the window's limit (include/fcd.h, fcd_set_crf_lattice_wide): up to 4096 states, walked in LDS beyond
    512 -- the labelling, the tile, the window's three rows and the S * N row within 160 KiB -- to the same bounds with
    ceil(states / 64) states per lane; a window within 512 states runs the same launches as wide=False.
    out: a float32 buffer of that shape (or (B, T, S, N) when n_hyp is 1) with dense (S, N) rows, written in place and
    returned; required with accumulate=True.  The call writes scale * occupancy, or adds it to what `out` holds with
    accumulate=True.  Rows at and beyond lengths[b], the blocks of labellings without a positive finite probability and
    of i >= n_valid[b] are not touched (zeros where the call allocates).  time_major_out: the array the call allocates is
    (T, B, n_hyp, S, N) and its (B, n_hyp, T, S, N) view is returned.
    Device tensors in: torch tensors on the same device, enqueued on torch's current stream, not synchronised.
    numpy in: numpy out."""
    return _lattice_call("crf", "occupancy", network_outputs, labels, label_lengths, lengths, paths, band, n_valid,
                         input_dtype, handle, init_states, wide=wide, out=out, scale=scale, accumulate=accumulate,
                         time_major_out=time_major_out)


def ctc_occupancy_batch_raw(network_outputs, labels, label_lengths, collapse_repeats=True, lengths=None, paths=None, band=0,
                            n_valid=None, out=None, scale=1.0, accumulate=False, time_major_out=False, input_dtype=None,
                            handle=None, wide=False):
    """The label occupancies of every labelling under plain CTC: occupancy[b][i][t][c] is the probability, over the
    alignments of labelling (b, i) to its read, that row t emits symbol c (0: the blank) -- the soft version of
    ctc_align_batch_raw's spans, and the gradient of ln P(labelling | x) by ln x[t][c]: at the logits of a softmax the
    gradient of -ln P is softmax - occupancy (include/fcd.h, fcd_ctc_occupancy_*; ctc_loss is that composition).
    -> OccupancyResult with occupancy (B, n_hyp, T, N) float32 and logp (B, n_hyp) float64, ctc_score's value bit for bit.
    For every labelling with a finite logp every row t < lengths[b] sums to 1.  The walks keep one float32 exponent per
    row: a long read that does not support its labelling (near-uniform posteriors, many rows per label) is outside what
    they hold; the walk checks every row's sum and gives such a labelling up -- logp NaN and NaN in its rows -- rather than
    return occupancies that do not add up (include/fcd.h has the rule, INTEGRATION.md section 2n the measured range).

    Arguments as ctc_posterior_batch_raw, and its limits: windows of at most 510 states (bands up to 126, exact mode up to
    254 rows or labels) and N - 1 <= 8.  wide=True lifts the first limit (include/fcd.h, fcd_set_ctc_occupancy_wide): every
    labelling ctc_score takes, N - 1 <= 8 -- a window beyond 510 states is walked in LDS (up to 10240 states; the
    labelling, the tile and two rows of the window within 160 KiB), to bound_w / lost_w of include/fcd.h; a window within
    510 states runs the same launches and returns the same bits as wide=False.  out: a float32 buffer of that shape (or (B, T, N), the shape of the input, when
    n_hyp is 1) with dense rows of N, written in place and returned; required with accumulate=True.  The call writes
    scale * occupancy, or adds it to what `out` holds with accumulate=True: out=softmax.clone(), scale=-1,
    accumulate=True leaves the logit gradient of -ln P.  Rows at and beyond lengths[b], the blocks of labellings without a
    positive finite probability and of i >= n_valid[b] are not touched (zeros where the call allocates).  time_major_out:
    the array the call allocates is (T, B, n_hyp, N) and its (B, n_hyp, T, N) view is returned.
    Device tensors in: torch tensors on the same device, enqueued on torch's current stream, not synchronised.
    numpy in: numpy out."""
    return _lattice_call("ctc", "occupancy", network_outputs, labels, label_lengths, lengths, paths, band, n_valid,
                         input_dtype, handle, collapse_repeats=collapse_repeats, wide=wide, out=out, scale=scale,
                         accumulate=accumulate, time_major_out=time_major_out)


def ctc_occupancy(network_output, sequence, alphabet, collapse_repeats=True, wide=False):
    """The label occupancies of one string against one (T, N) float32 posterior matrix, exact lattice: -> (occupancy,
    logp) with occupancy a (T, N) float32 array (entry [t][c]: the probability, over the string's alignments, that row t
    emits alphabet[c]; every row sums to 1) and logp = ln P(sequence | network_output).  RuntimeError where the string has
    no alignment of positive finite probability.  Argument checks as ctc_score.  wide: as ctc_occupancy_batch_raw --
    strings beyond 254 rows or characters."""
    x, lab, n, _ = _ctc_one_read(network_output, sequence, alphabet, "ctc_occupancy")
    r = ctc_occupancy_batch_raw(x, lab, n, collapse_repeats, wide=wide)
    logp = float(r.logp[0, 0])
    if not np.isfinite(logp):
        raise RuntimeError("ctc_occupancy: the sequence has no alignment of positive finite probability (ln P = %r)" % logp)
    return r.occupancy[0, 0].copy(), logp


_CTC_LOSS_FN = []


def _ctc_loss_function():
    if _CTC_LOSS_FN:
        return _CTC_LOSS_FN[0]
    import torch

    class CtcLoss(torch.autograd.Function):
        @staticmethod
        def forward(ctx, log_probs, labels, label_lengths, lengths, collapse_repeats, paths, band):
            probs = log_probs.detach().exp()
            occ = ctc_occupancy_batch_raw(probs, labels, label_lengths, collapse_repeats, lengths, paths, band, scale=-1.0,
                                          wide=True)
            logp = occ.logp[:, 0]
            ctx.save_for_backward(occ.occupancy[:, 0], logp)  # -occupancy: zeros beyond lengths[b] and where P = 0
            ctx.in_dtype = log_probs.dtype
            return -logp

        @staticmethod
        def backward(ctx, grad_loss):
            neg_occ, logp = ctx.saved_tensors
            g = grad_loss.to(torch.float32)[:, None, None] * neg_occ
            # (a given-up labelling holds NaN already; any other NaN loss has a NaN gradient too -- selected on the device)
            g = torch.where(torch.isnan(logp)[:, None, None], torch.full_like(g, float("nan")), g)
            return g.to(ctx.in_dtype), None, None, None, None, None, None

    _CTC_LOSS_FN.append(CtcLoss.apply)
    return CtcLoss.apply


def ctc_loss(log_probs, labels, label_lengths, lengths=None, collapse_repeats=True, paths=None, band=0):
    """The CTC training loss on ctc_score's own lattice.  log_probs: (B, T, N) log-posteriors (the output of log_softmax), a
    torch ROCm tensor (float32 / float16 / bfloat16) of any non-negative strides -- a (T, B, N) tensor's .permute(1, 0, 2)
    is taken as it is; labels (B, Lmax) uint8 with values 1 .. N-1, label_lengths (B,); lengths (B,) rows per read.
    -> loss (B,) float64, differentiable:  loss_b = -ln P(y_b | x_b), ctc_score_batch_raw's value negated.  The caller
    reduces.  collapse_repeats=False, and band=W > 0 with paths (the banded sum and its own exact gradient), as ctc_score.

    Forward: one elementwise exp, then one ctc_occupancy_batch_raw call, which yields ln P and the occupancies that are
    saved.  Backward: grad_log_probs = -grad_out[:, None, None] * occupancy in the dtype of log_probs, 0 on rows at and
    beyond lengths[b]; no loop over rows or reads, nothing synchronises.  A read without an alignment (P = 0: more labels
    than rows) has loss +inf and gradient 0; a labelling the occupancy walk gives up (a long read that does not support it:
    ctc_occupancy_batch_raw) has a NaN loss and a NaN gradient, as has a NaN posterior or a label outside 1 .. N-1.
    Limits: ctc_occupancy_batch_raw's with wide=True -- every labelling ctc_score takes at N - 1 <= 8: windows of up to
    10240 states (exact: 5119 rows or labels; any band up to 2559) whose labelling, tile and two rows fit the 160 KiB of
    LDS.  Up to 510 states (254 labels, band 126) the register-resident walk runs, as before; beyond, the LDS-resident one
    (INTEGRATION.md section 2o)."""
    if not _is_torch_cuda(log_probs):
        raise TypeError("ctc_loss takes a torch ROCm tensor")
    if log_probs.ndim != 3:
        raise TypeError("expected a tensor of rank 3")
    if getattr(labels, "ndim", 2) != 2:
        raise ValueError("labels must have shape (n_reads, Lmax): one labelling per read")
    return _ctc_loss_function()(log_probs, labels, label_lengths, lengths, bool(collapse_repeats), paths, band)


def _crf_sequence_labels(sequence, alpha, what):
    """The labels behind a string crf_beam_search built: it joins the labels' strings leaf to root and reverses the
    CHARACTERS (src/search.rs:146-156), so a multi-character label appears reversed."""
    if not isinstance(sequence, str):
        raise TypeError("argument 'sequence': expected str")
    index = {}
    for i, a in enumerate(alpha):
        if i > 0 and a:
            index.setdefault(a[::-1], i)
    width = sorted({len(a) for a in index}, reverse=True)
    out, pos = [], 0
    while pos < len(sequence):
        for w in width:  # (the longest label first: an alphabet whose labels prefix one another is read greedily)
            lab = index.get(sequence[pos:pos + w])
            if lab is not None:
                out.append(lab)
                pos += w
                break
        else:
            raise ValueError("%s: sequence holds %r, which is not a label of the alphabet" % (what, sequence[pos]))
    return out


def _crf_one_read(network_output, init_state, sequence, alphabet, what):
    x = _as_f32(network_output, 3, "network_output")
    init = _as_f32(init_state, 1, "init_state")
    alpha = _seq_to_vec(alphabet)
    _check_greedy_alphabet(len(alpha), x.shape[2])
    if init.size == 0:
        raise RuntimeError("init_state is empty")
    y = _crf_sequence_labels(sequence, alpha, what)
    lab = np.zeros((1, max(len(y), 1)), np.uint8)
    lab[0, :len(y)] = y
    return _dense(x)[None], np.ascontiguousarray(init)[None], lab, np.array([len(y)], np.uint32), len(y)


def crf_score(network_output, init_state, sequence, alphabet, wide=False):
    """ln P(sequence | network_output) under the CRF model: every alignment of one string (as crf_beam_search returns
    it) to one (T, S, N) float32 posterior array, exact, as a float.  More than 511 labels: RuntimeError -- unless
    wide=True (crf_score_batch_raw: up to 4095 rows or labels)."""
    x, init, lab, n, _ = _crf_one_read(network_output, init_state, sequence, alphabet, "crf_score")
    return float(crf_score_batch_raw(x, init, lab, n, wide=wide)[0, 0])


def crf_align(network_output, init_state, sequence, alphabet):
    """The best alignment of one string to one (T, S, N) float32 posterior array under the CRF model, exact:
    -> (rows, quals, logp), the row each label is emitted at, the posterior of that emission and ln of the alignment's
    probability.  No alignment: ([], [], -inf or NaN).  More than 511 labels: RuntimeError."""
    x, init, lab, n, L = _crf_one_read(network_output, init_state, sequence, alphabet, "crf_align")
    r = crf_align_batch_raw(x, init, lab, n)
    logp = float(r.logp[0, 0])
    if not np.isfinite(logp):
        return [], [], logp
    return [int(s) for s in r.start[0, 0, :L]], [float(q) for q in r.qual[0, 0, :L]], logp


def crf_posterior(network_output, init_state, sequence, alphabet):
    """The substitution posteriors of one string (as crf_beam_search returns it) against one (T, S, N) float32 posterior
    array under the CRF model, exact lattice: -> (post, logp) with post an (L, N-1) float32 array (row k: the posterior
    over alphabet[1:] at label k) and logp = ln P(sequence | network_output).  Argument checks as crf_score."""
    x, init, lab, n, L = _crf_one_read(network_output, init_state, sequence, alphabet, "crf_posterior")
    r = crf_posterior_batch_raw(x, init, lab, n)
    return r.post[0, 0, :L].copy(), float(r.logp[0, 0])


def crf_edits(network_output, init_state, sequence, alphabet):
    """The deletion and insertion likelihoods of one string (as crf_beam_search returns it) against one (T, S, N) float32
    posterior array under the CRF model, exact lattice: -> (deletion, insertion, logp) with deletion an (L,) and insertion
    an (L + 1, N-1) float32 array of log-ratios (insertion[g, c - 1]: alphabet[c] inserted before label g) and logp =
    ln P(sequence | network_output).  Argument checks as crf_score."""
    x, init, lab, n, L = _crf_one_read(network_output, init_state, sequence, alphabet, "crf_edits")
    r = crf_edits_batch_raw(x, init, lab, n)
    return r.deletion[0, 0, :L].copy(), r.insertion[0, 0, :L + 1].copy(), float(r.logp[0, 0])


def crf_occupancy(network_output, init_state, sequence, alphabet, wide=False):
    """The edge occupancies of one string (as crf_beam_search returns it) against one (T, S, N) float32 posterior array
    under the CRF model, exact lattice: -> (occupancy, logp) with occupancy a (T, S, N) float32 array (entry [t][s][a]: the
    probability, over the string's alignments, of leaving state s by alphabet[a] at row t; every row sums to 1) and logp =
    ln P(sequence | network_output).  RuntimeError where the string has no alignment of positive finite probability.
    Argument checks as crf_score; wide as crf_occupancy_batch_raw -- strings beyond 511 rows or characters."""
    x, init, lab, n, _ = _crf_one_read(network_output, init_state, sequence, alphabet, "crf_occupancy")
    r = crf_occupancy_batch_raw(x, init, lab, n, wide=wide)
    logp = float(r.logp[0, 0])
    if not np.isfinite(logp):
        raise RuntimeError("crf_occupancy: the sequence has no alignment of positive finite probability (ln P = %r)" % logp)
    return r.occupancy[0, 0].copy(), logp


# ---------------------------------------------------------------------------------------------
# beam-search sessions (include/fcd.h, fcd_beam_session_*): the 1-D beam searches advanced over rows as they arrive
# ---------------------------------------------------------------------------------------------
class _CrfBatchResult(BatchResult):
    """A BatchResult whose strings follow crf_beam_search_batch's character handling (multi-character labels reversed)."""

    def cpu(self):
        r = BatchResult.cpu(self)
        return _CrfBatchResult(r.labels, r.path, r.out_len, r.status, r.qual, r.ambiguous)

    def sequences(self, alphabet, raise_on_error=True, paths="list"):
        r = self.cpu()
        alpha = _seq_to_vec(alphabet)
        out = BatchResult.sequences(r, alpha, raise_on_error, paths)
        for i, item in enumerate(out):
            if item is not None:
                labels = r.labels[i, :int(r.out_len[i])]
                out[i] = ("".join(alpha[l] for l in labels[::-1])[::-1], item[1])
        return out


class _CrfViterbiResult(_CrfBatchResult):
    """crf_viterbi_search_batch_raw's result: a CRF batch result with logp, (n_reads,) float64 -- ln of the probability of
    the best state path (NaN for a read that failed)."""

    def __init__(self, labels, path, out_len, status, qual=None, ambiguous=None, logp=None):
        _CrfBatchResult.__init__(self, labels, path, out_len, status, qual, ambiguous)
        self.logp = logp

    def sequences(self, alphabet, raise_on_error=True, paths="list"):
        """-> list of (str, path) per read: crf_greedy_search's strings (labels joined in order), which is what
        crf_viterbi_search and crf_viterbi_search_batch return -- not crf_beam_search_batch's handling of multi-character
        labels, which the other CRF results follow."""
        return BatchResult.sequences(self, alphabet, raise_on_error, paths)

    def cpu(self):
        r = BatchResult.cpu(self)  # (joins the handle's internal streams first)
        return _CrfViterbiResult(r.labels, r.path, r.out_len, r.status, r.qual, r.ambiguous, _to_host(self.logp))


class BeamSearchSession:
    """A fixed set of n_reads read slots whose search::beam_search advances over the rows pushed to it (include/fcd.h,
    fcd_beam_session_*).  The result of a slot is, at any time, exactly what beam_search_batch_raw returns for all the rows
    pushed to it since creation or its restart; a failed slot stays failed.

        s = BeamSearchSession(n_reads, n_labels, max_steps, beam_size=5, beam_cut_threshold=0.1)
        s.push(chunk)                      # (n_reads, T_c, N): torch ROCm tensor, DLPack device array or numpy
        r = s.push(chunk, lengths, result=True)   # the result after the push, from the same launch
        r = s.result()                     # BatchResult, out_stride = max_steps; .cpu(), .sequences(alphabet)
        s.restart([3, 7])                  # slots 3 and 7 start a new read

    Device chunks run on torch's current stream and return torch tensors; numpy chunks are uploaded by the library and
    return numpy arrays (result(host=...) chooses; by default it follows the last push).  `lengths` is a host sequence
    (a device tensor is copied to the host first, which synchronises).  The session keeps the device chunks it was given
    until their push has run.  max_steps: the most rows a slot takes between restarts; a push past it raises ValueError and
    changes nothing.  Memory: one device allocation made at creation (nbytes)."""
    _crf = False

    def __init__(self, n_reads, n_labels, max_steps, beam_size=5, beam_cut_threshold=0.0, collapse_repeats=True,
                 count_ambiguous=False, kernel=nat.KERNEL_AUTO, device=0, handle=None):
        self._open(n_reads, n_labels, 1, max_steps, count_ambiguous, device, handle)
        self._h.check(self._lib.fcd_beam_session_create(
            self._h.ptr, self.n_reads, self.n_labels, self.max_steps, int(beam_size), float(beam_cut_threshold),
            int(bool(collapse_repeats)), int(kernel), int(bool(count_ambiguous)), C.byref(self._ptr)))

    def _open(self, n_reads, n_labels, n_states, max_steps, count_ambiguous, device, handle):
        self._h = handle if handle is not None else nat.default_handle(device)
        self._lib = self._h.lib
        self._ptr = C.c_void_p()
        self.n_reads, self.n_labels, self.n_states = int(n_reads), int(n_labels), int(n_states)
        self.max_steps = int(max_steps)
        self.count_ambiguous = bool(count_ambiguous)
        self._host_mode = None  # the kind of the last push's chunk
        self._held = []         # (event, tensors) of device pushes that may not have run yet

    def _check_rc(self, rc):
        if rc == nat.E_INVALID:
            msg = self._lib.fcd_last_error(self._h.ptr)
            raise ValueError(msg.decode() if msg else "invalid argument")
        self._h.check(rc)

    def _lengths(self, lengths):
        if lengths is None:
            return None
        if hasattr(lengths, "cpu"):
            lengths = lengths.cpu()  # (a device tensor: synchronises)
        l = np.ascontiguousarray(np.asarray(lengths), np.int64)
        if l.shape != (self.n_reads,):
            raise ValueError("lengths must have shape (n_reads,)")
        return l

    def _init_rows(self, init_states, n):
        if hasattr(init_states, "cpu"):
            init_states = init_states.cpu()
        init = np.ascontiguousarray(np.asarray(init_states, np.float32))
        if init.ndim != 2 or init.shape[0] != n or init.shape[1] < 1:
            raise ValueError("init_states must have shape (%d, n_init)" % n)
        return init

    def _result_arrays(self, host, like=None):
        B, W = self.n_reads, self.max_steps
        if host:
            out = _HostOut(B, W, want_amb=self.count_ambiguous)
            return out.res, (out.labels, out.path, out.out_len, out.status, None, out.ambiguous)
        import torch
        dev = like.device if like is not None else torch.device("cuda", self._h.device)
        labels = torch.empty((B, W), dtype=torch.uint8, device=dev)
        path = torch.empty((B, W), dtype=torch.int32, device=dev)
        meta = torch.empty((2, B), dtype=torch.int32, device=dev)
        amb = torch.empty((B, 2), dtype=torch.int32, device=dev) if self.count_ambiguous else None
        res = nat.Result(labels.data_ptr(), path.data_ptr(), None, meta[0].data_ptr(), meta[1].data_ptr(), W,
                         amb.data_ptr() if amb is not None else None)
        self._h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        return res, (labels, path, meta[0], meta[1], None, amb)

    def _wrap(self, arrays):
        r = (_CrfBatchResult if self._crf else BatchResult)(*arrays)
        return r

    def _hold(self, tensors):
        import torch
        self._held = [(e, t) for e, t in self._held if not e.query()]
        e = torch.cuda.Event()
        e.record(torch.cuda.current_stream(tensors[0].device))
        self._held.append((e, tensors))

    def push(self, chunk, lengths=None, result=False, input_dtype=None):
        """Slot r takes the first lengths[r] rows of `chunk` (all of them if lengths is None; 0 leaves it untouched).
        result=True: returns the BatchResult after the push (one launch), else None."""
        if not self._ptr:
            raise ValueError("the session is closed")
        l = self._lengths(lengths)
        ndim = 4 if self._crf else 3
        dev_x = _device_tensor(chunk)
        if dev_x is None:
            x = _dense(np.asarray(chunk))
            if x.ndim != ndim or x.dtype not in (np.float32, np.float16, np.uint16):
                raise TypeError("expected a float32 (or float16 / bfloat16-bits uint16) array of rank %d" % ndim)
            if x.shape[0] != self.n_reads:
                raise ValueError("the chunk must have n_reads = %d rows of reads" % self.n_reads)
            b = _host_batch(x, self._crf, l, input_dtype)
            res, arrays = self._result_arrays(True) if result else (None, None)
            self._check_rc(self._lib.fcd_beam_session_push_host(self._ptr, C.byref(b), C.byref(res) if result else None))
            self._host_mode = True
            return self._wrap(arrays) if result else None
        import torch
        x = dev_x
        if x.dim() != ndim or x.shape[0] != self.n_reads:
            raise ValueError("expected a (n_reads, T_c, %s) device tensor" % ("S, N" if self._crf else "N"))
        st = x.stride()
        if self._crf:
            b = nat.Batch(x.data_ptr(), x.shape[0], x.shape[1], x.shape[2], x.shape[3], st[0], st[1], st[2], st[3], None,
                          _torch_dtype_code(x))
        else:
            b = nat.Batch(x.data_ptr(), x.shape[0], x.shape[1], 1, x.shape[2], st[0], st[1], 0, st[2], None,
                          _torch_dtype_code(x))
        if l is not None:
            b.lengths = l.ctypes.data
        if result:
            res, arrays = self._result_arrays(False, x)
        else:
            res, arrays = None, None
            self._h.set_stream(torch.cuda.current_stream(x.device).cuda_stream)
        self._check_rc(self._lib.fcd_beam_session_push_dev(self._ptr, C.byref(b), C.byref(res) if result else None))
        self._hold((x,))
        self._host_mode = False
        return self._wrap(arrays) if result else None

    def result(self, host=None):
        """BatchResult of every slot's prefix (the session does not change).  host=None: numpy arrays if the last push
        was a numpy chunk (or, before any push, if no ROCm device is visible to torch), torch tensors otherwise."""
        if not self._ptr:
            raise ValueError("the session is closed")
        if host is None:
            host = self._host_mode
            if host is None:
                try:
                    import torch
                    host = not torch.cuda.is_available()
                except ImportError:
                    host = True
        res, arrays = self._result_arrays(bool(host))
        fn = self._lib.fcd_beam_session_result_host if host else self._lib.fcd_beam_session_result_dev
        self._check_rc(fn(self._ptr, C.byref(res)))
        return self._wrap(arrays)

    def restart(self, slots, init_states=None):
        """The listed slots go back to the root with 0 steps (CRF: each with a new init row, init_states[j] for slots[j])."""
        s = np.ascontiguousarray(np.asarray(slots, np.int64).reshape(-1))
        init = None
        if self._crf:
            if init_states is None:
                raise ValueError("a CRF session restarts a slot with a new init row")
            init = self._init_rows(init_states, len(s))
            if init.shape[1] != self._n_init:
                raise ValueError("init rows must have %d entries" % self._n_init)
        self._check_rc(self._lib.fcd_beam_session_restart(self._ptr, s.ctypes.data, len(s),
                                                          init.ctypes.data if init is not None else None))

    @property
    def steps(self):
        """rows each slot has taken since creation or its restart (numpy int64, n_reads)"""
        out = np.zeros(self.n_reads, np.int64)
        self._h.check(self._lib.fcd_beam_session_steps(self._ptr, out.ctypes.data))
        return out

    @property
    def nbytes(self):
        return int(self._lib.fcd_beam_session_bytes(self._ptr))

    def close(self):
        if self._ptr:
            self._lib.fcd_beam_session_destroy(self._ptr)
            self._ptr = C.c_void_p()
            self._held = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CrfBeamSearchSession(BeamSearchSession):
    """BeamSearchSession of search::crf_beam_search: chunks are (n_reads, T_c, S, N); init_states (n_reads, n_init) are
    the slots' first init rows (a NaN row, or a state the table does not hold, fails the slot at its first non-empty
    push).  Strings follow crf_beam_search_batch's character handling."""
    _crf = True

    def __init__(self, n_reads, n_states, n_labels, init_states, max_steps, beam_size=5, beam_cut_threshold=0.0,
                 count_ambiguous=False, kernel=nat.KERNEL_AUTO, device=0, handle=None):
        self._open(n_reads, n_labels, n_states, max_steps, count_ambiguous, device, handle)
        init = self._init_rows(init_states, self.n_reads)
        self._n_init = init.shape[1]
        self._check_rc(self._lib.fcd_crf_beam_session_create(
            self._h.ptr, self.n_reads, self.n_states, self.n_labels, init.ctypes.data, self._n_init, self.max_steps,
            int(beam_size), float(beam_cut_threshold), int(kernel), int(bool(count_ambiguous)), C.byref(self._ptr)))
