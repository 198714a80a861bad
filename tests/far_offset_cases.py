"""TEST INFRASTRUCTURE shared by tests/test_far_offsets_emu.py (the kernels on the wave64 emulator) and
tests/test_gpu_far_offsets.py (on the GPU): every entry point of the C ABI on layouts whose element offsets pass 2^31 and
whose byte offsets pass 2^32.

The technique: one UNINITIALISED backing buffer per array (np.empty on the CPU, a slice of one torch.empty pool on the GPU),
of which only the few KiB a case reads are ever written -- untouched pages are never committed.  The calls go through the
*_dev entry points with raw pointers and explicit strides (on the emulator device memory is host memory).

Every case runs the same inputs twice, COMPACT (the layout the other tests use) and FAR, and asserts
  1. the compact result against the family's reference: the oracle for the searches, the float64 restatements for
     crf_viterbi_search and the lattice families, with those families' own bounds;
  2. far == compact EXACTLY wherever the kernel is documented to write (status, out_len, labels, path, and quality / score /
     logp / posterior / edit values as bit patterns).
"Far" always means: read, row or labelling 1 starts beyond the boundary while read 0 starts at offset 0.

What the table holds: the searches (far reads, far rows, far outputs), sessions, the duplex searches and the band estimator,
pack / offsets / unpack, the tree arena; the ten lattice entry points -- ctc / crf x score, align, posterior, edits,
occupancy -- with far labellings (y.stride), far reads and far rows, and the occupancy blocks far apart (stride_row) or
interleaved with far rows (stride_t), written and accumulated, in one launch group and in one per read; the two walks over
all labellings (crf_transition_probs, crf_marginals) with each of their strides far alone, in every code form, both score
layouts and both output types.  ONE quantity is far per case, so that a failure names the offset that broke.  COVERED and
EXEMPT (at the end) list every fcd_*_dev of include/fcd.h; tests/test_far_offsets_emu.py holds the header to them.

Memory: Env.region() hands out the big arrays; on the GPU they are slices of ONE pool made once per module (never filled,
never copied as a whole: put() and get() move the touched rows only), on the CPU an np.empty each, dropped by reset()."""
import ctypes as C

import numpy as np

from kat_cases import reference_style_rows
from oracle import oracle

N = 5
ESIZE = {"f32": 4, "f16": 2, "bf16": 2}
DTYPE_CODE = {"f32": 0, "f16": 1, "bf16": 2}
PATTERN = 0xEE
STRIP = 64  # entries after row 0's T that the far-output cases fill with PATTERN and find untouched


def nat():
    from fast_ctc_decode_amd import _native
    return _native


# ---- memory ----------------------------------------------------------------------------------------------------------
class Region:
    """nbytes of uninitialised memory at .ptr (256-byte aligned); put / get move only the bytes named"""

    def __init__(self, env, nbytes):
        self.env, self.nbytes = env, int(nbytes)
        if env.device is None:
            self._a = np.empty(self.nbytes + 256, np.uint8)
            self._off = (-self._a.ctypes.data) % 256
            self.ptr = self._a.ctypes.data + self._off
        else:
            self._off = env._take(self.nbytes)
            self._a = env.pool
            self.ptr = env.pool.data_ptr() + self._off

    def put(self, byte_off, arr):
        raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        lo = self._off + int(byte_off)
        assert 0 <= byte_off and byte_off + raw.size <= self.nbytes, (byte_off, raw.size, self.nbytes)
        if self.env.device is None:
            self._a[lo:lo + raw.size] = raw
        else:
            import torch
            self._a[lo:lo + raw.size].copy_(torch.from_numpy(raw.copy()))

    def fill(self, byte_off, nbytes, value=PATTERN):
        self.put(byte_off, np.full(int(nbytes), value, np.uint8))

    def get(self, byte_off, dtype, count):
        n = int(count) * np.dtype(dtype).itemsize
        lo = self._off + int(byte_off)
        assert 0 <= byte_off and byte_off + n <= self.nbytes, (byte_off, n, self.nbytes)
        if self.env.device is None:
            return self._a[lo:lo + n].copy().view(dtype)
        return self._a[lo:lo + n].cpu().numpy().view(dtype)


class Env:
    """where a case's arrays live and the handle its calls go through.  device None: the emulator (host memory);
    "cuda": slices of `pool`, a uint8 tensor made once by the caller and never filled."""

    def __init__(self, device=None, pool=None):
        self.device, self.pool = device, pool
        self._used = 0
        self.h = nat().default_handle() if device is None else nat().default_handle(0)
        self.lib = self.h.lib
        if device is not None:
            import torch
            self.h.set_stream(torch.cuda.current_stream().cuda_stream)

    def _take(self, nbytes):
        """from the pool's END downwards: an offset that lost its upper bits, or went negative, then points into the pool
        below the region -- a mismatch the comparison reports, not an access outside the allocation"""
        end = self.pool.numel() - self._used
        off = (end - nbytes) - (self.pool.data_ptr() + end - nbytes) % 256
        assert off >= 0, ("the pool is too small", nbytes, self._used, self.pool.numel())
        self._used = self.pool.numel() - off
        return off

    def reset(self):
        """forget every region (the GPU's pool is reused from its start)"""
        self.sync()
        self._used = 0

    def region(self, nbytes):
        return Region(self, nbytes)

    def small(self, arr):
        arr = np.ascontiguousarray(arr)
        r = Region(self, max(arr.nbytes, 1))
        if arr.nbytes:
            r.put(0, arr)
        r.dtype, r.count = arr.dtype, arr.size
        return r

    def sync(self):
        self.h.synchronize()
        if self.device is not None:
            import torch
            torch.cuda.synchronize()

    def workspace_bytes(self):
        return self.h.workspace_bytes()

    def close(self):
        self.sync()
        if self.device is not None:
            self.h.reset_stream()


# ---- inputs ----------------------------------------------------------------------------------------------------------
def to_dtype(x, dtype):
    """-> (the array the kernels read, its exact float32 upcast)"""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "f16":
        xin = x.astype(np.float16)
        return xin, xin.astype(np.float32)
    if dtype == "bf16":
        bits = (x.view(np.uint32) >> 16).astype(np.uint16)  # truncation: any bf16 value will do
        return bits, (bits.astype(np.uint32) << 16).view(np.float32)
    return x, x


def plain_reads(seed, B, T, dtype):
    rng = np.random.default_rng(seed)
    return to_dtype(reference_style_rows(rng, B * T, N).reshape(B, T, N), dtype)


def crf_reads(seed, B, T, S, dtype, floor=False):
    """Dirichlet-like rows; floor: floored at 2^-20 on the array the kernels read (crf_viterbi_search's condition)"""
    rng = np.random.default_rng(seed)
    if floor:
        import crf_viterbi_reference as VR
        x = np.stack([VR.random_case(rng, T, S, N)[0] for _ in range(B)])
    else:
        x = rng.random((B, T, S, N), dtype=np.float32)
        x /= x.sum(-1, keepdims=True)
    xin, x32 = to_dtype(x, dtype)
    if floor:
        assert (x32 >= 2.0 ** -20).all()
    init = rng.random((B, S)).astype(np.float32)
    return xin, x32, init


def ragged(B, T):
    """lengths T and T - 3 in turn: every far read ends inside a tile"""
    return np.array([T if b % 2 == 0 else T - 3 for b in range(B)], np.int64)


class Layout:
    """strides of a batch in elements; compact read-major when both are None"""

    def __init__(self, stride_read=None, stride_t=None):
        self.stride_read, self.stride_t = stride_read, stride_t

    def strides(self, T, inner):
        st = inner if self.stride_t is None else self.stride_t
        sr = T * inner if self.stride_read is None else self.stride_read
        return sr, st


def place_batch(env, xin, layout, dtype, lengths, S=1):
    """-> (nat.Batch, [regions to keep alive]): xin (B, T, inner...) written row block by row block at the layout's strides"""
    B, T = xin.shape[:2]
    inner = int(np.prod(xin.shape[2:]))
    e = ESIZE[dtype]
    sr, st = layout.strides(T, inner)
    span = (B - 1) * sr + (T - 1) * st + inner
    reg = env.region(span * e)
    flat = xin.reshape(B, T, inner)
    if st == inner:          # a read is one block
        for b in range(B):
            reg.put(b * sr * e, flat[b])
    elif sr == inner:        # time-major: a time step is one block
        for t in range(T):
            reg.put(t * st * e, flat[:, t])
    else:
        for b in range(B):
            for t in range(T):
                reg.put((b * sr + t * st) * e, flat[b, t])
    ln = env.small(lengths)
    nn = xin.shape[-1]
    batch = nat().Batch(reg.ptr, B, T, S, nn, sr, st, nn if S > 1 else 0, 1, ln.ptr, DTYPE_CODE[dtype])
    return batch, [reg, ln]


SLOT = 64 * 1024  # far layouts: the arrays of a call share ONE span, each starting a slot after the other -- their rows
                  # (a few hundred bytes each) never meet, and the span is as large as the widest array alone


class _Sub:
    """a part of a region, with the region's put / get"""

    def __init__(self, reg, off):
        self.reg, self.off, self.ptr = reg, off, reg.ptr + off

    def put(self, byte_off, arr):
        self.reg.put(self.off + byte_off, arr)

    def get(self, byte_off, dtype, count):
        return self.reg.get(self.off + byte_off, dtype, count)

    def fill(self, byte_off, nbytes, value=PATTERN):
        self.reg.fill(self.off + byte_off, nbytes, value)


# ---- outputs ---------------------------------------------------------------------------------------------------------
class Out:
    """the arrays of an fcd_result of `rows` rows at `out_stride`: labels / path / qual are regions of which row 0 and its
    strip are PATTERN-filled beforehand when the layout is far"""

    def __init__(self, env, B, T, out_stride=None, path=True, qual=False, ambiguous=False, rows=None, logp=False, nbest=0):
        self.env, self.B, self.T = env, B, T
        self.rows = rows = B if rows is None else rows
        self.W = W = T if out_stride is None else out_stride
        self.far = out_stride is not None
        span = (rows - 1) * W + T + STRIP
        if self.far and W >= 2 ** 24:  # the three arrays share ONE span, a slot apart: their rows (a few hundred bytes) never meet
            whole = env.region(span * (4 if path or qual else 1) + 3 * SLOT)
            self.labels = _Sub(whole, 0)
            self.path = _Sub(whole, SLOT) if path else None
            self.qual = _Sub(whole, 2 * SLOT) if qual else None
        else:
            self.labels = env.region(span)
            self.path = env.region(span * 4) if path else None
            self.qual = env.region(span * 4) if qual else None
        if self.far:
            for reg, e in ((self.labels, 1), (self.path, 4), (self.qual, 4)):
                if reg is not None:
                    reg.fill(0, (T + STRIP) * e)
        self.out_len = env.small(np.full(rows, 0x7777, np.uint32))
        self.status = env.small(np.full(B, -7, np.int32))
        self.amb = env.small(np.full((B, 2), 0x7777, np.uint32)) if ambiguous else None
        self.logp = env.small(np.full(B, 7.0)) if logp else None
        self.score = env.small(np.full(rows, 7.0, np.float32)) if nbest else None
        self.n_hyp = env.small(np.full(B, 0x7777, np.uint32)) if nbest else None
        self.nbest = nbest
        self.parks = False  # crf_viterbi_search: entries at and beyond out_len are unspecified up to the row's T (fcd.h)
        self.result = nat().Result(self.labels.ptr, self.path.ptr if path else None, self.qual.ptr if qual else None,
                                   self.out_len.ptr, self.status.ptr, W, self.amb.ptr if ambiguous else None)
        self.nb = nat().NBest(nbest, self.score.ptr, self.n_hyp.ptr) if nbest else None

    def read(self):
        """-> Got: numpy copies of every row's first T entries, and the bytes after row 0 that must be untouched"""
        self.env.sync()
        g = Got()
        T, W, rows = self.T, self.W, self.rows
        g.out_len = self.out_len.get(0, np.uint32, rows)
        g.status = self.status.get(0, np.int32, self.B)
        g.labels = np.stack([self.labels.get(r * W, np.uint8, T) for r in range(rows)])
        g.path = None if self.path is None else np.stack([self.path.get(r * W * 4, np.uint32, T) for r in range(rows)])
        g.qual = None if self.qual is None else np.stack([self.qual.get(r * W * 4, np.float32, T) for r in range(rows)])
        g.ambiguous = None if self.amb is None else self.amb.get(0, np.uint32, 2 * self.B).reshape(self.B, 2)
        g.logp = None if self.logp is None else self.logp.get(0, np.float64, self.B)
        g.score = None if self.score is None else self.score.get(0, np.float32, rows)
        g.n_hyp = None if self.n_hyp is None else self.n_hyp.get(0, np.uint32, self.B)
        if self.far:  # row 0 beyond out_len[0], and the strip behind it: not written
            n0 = T if self.parks else int(g.out_len[0])
            assert n0 <= T
            for name, reg, e in (("labels", self.labels, 1), ("path", self.path, 4), ("qual", self.qual, 4)):
                if reg is not None:
                    tail = reg.get(n0 * e, np.uint8, (T + STRIP - n0) * e)
                    assert (tail == PATTERN).all(), (name, "row 0 was written beyond out_len[0] =", n0,
                                                     np.flatnonzero(tail != PATTERN)[:8].tolist())
        return g


class Got:
    pass


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same(far, compact, where, fields=("labels", "path", "qual")):
    """far == compact wherever the kernel is documented to write; floats as bit patterns (NaNs equal)"""
    assert np.array_equal(far.status, compact.status), (where, "status", far.status, compact.status)
    assert np.array_equal(far.out_len, compact.out_len), (where, "out_len", far.out_len, compact.out_len)
    for r in range(len(compact.out_len)):
        n = int(compact.out_len[r])
        for f in fields:
            a, b = getattr(far, f), getattr(compact, f)
            if a is None or b is None:
                continue
            assert np.array_equal(bits(a[r, :n]), bits(b[r, :n])), (where, f, "row", r)
    for f in ("ambiguous", "logp", "score", "n_hyp"):
        a, b = getattr(far, f), getattr(compact, f)
        if a is not None and b is not None:
            assert np.array_equal(bits(a), bits(b)), (where, f, a, b)


# ---- the searches ----------------------------------------------------------------------------------------------------
class Search:
    """one entry point with its arguments: builds its inputs (once), calls the _dev entry point on a layout, checks a
    compact result against the family's reference"""
    crf = False
    qual = False
    ambiguous = False
    logp = False
    nbest = 0
    floor = False
    parks = False

    def __init__(self, name, S=1, **kw):
        self.name, self.S = name, S
        self.__dict__.update(kw)
        self._data = {}

    def data(self, B, T, dtype):
        key = (B, T, dtype)
        if key not in self._data:
            seed = 9000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(self.name)) + 31 * B + T + 7 * DTYPE_CODE[dtype]
            if self.crf:
                xin, x32, init = crf_reads(seed, B, T, self.S, dtype, self.floor)
            else:
                (xin, x32), init = plain_reads(seed, B, T, dtype), None
            d = dict(xin=xin, x32=x32, init=init, lengths=ragged(B, T), B=B, T=T, dtype=dtype)
            d["want"] = self.reference(d)
            self._data[key] = d
        return self._data[key]

    def run(self, env, d, layout=None, out_stride=None, path=True, qual=None, keep_out=False):
        layout = layout or Layout()
        B, T = d["B"], d["T"]
        batch, keep = place_batch(env, d["xin"], layout, d["dtype"], d["lengths"], self.S)
        init = env.small(d["init"]) if self.crf else None
        qual = self.qual if qual is None else (qual and self.qual)
        out = Out(env, B, T, out_stride, path, qual, self.ambiguous, B * self.nbest if self.nbest else None, self.logp, self.nbest)
        out.parks = self.parks
        rc = self.call(env, batch, init, out)
        assert rc == nat().OK, (self.name, rc, env.lib.fcd_last_error(env.h.ptr))
        got = out.read()
        del keep
        return (got, out) if keep_out else got

    # (filled in by the subclasses)
    def call(self, env, batch, init, out):
        raise NotImplementedError

    def reference(self, d):
        raise NotImplementedError

    def check(self, got, d):
        raise NotImplementedError


class Viterbi(Search):
    qual = True

    def call(self, env, batch, init, out):
        return env.lib.fcd_viterbi_search_dev(env.h.ptr, C.byref(batch), self.collapse, C.byref(out.result))

    def reference(self, d):
        return [oracle.viterbi_search_raw(np.ascontiguousarray(d["x32"][b, :d["lengths"][b]]), bool(self.collapse))
                for b in range(d["B"])]

    def check(self, got, d):
        for b, (labels, path, quals) in enumerate(d["want"]):
            n = int(got.out_len[b])
            assert int(got.status[b]) == 0 and n == len(labels), (self.name, b)
            assert np.array_equal(got.labels[b, :n], labels) and np.array_equal(got.path[b, :n], path), (self.name, b)
            if got.qual is not None:
                assert [ord(oracle.lib.fcdo_phred(float(q), 1.0, 0.0)) for q in got.qual[b, :n]] == list(quals), (self.name, b)


class Beam(Search):
    """beam_search on the kernel AUTO picks for the beam (5: wave, 24: lane, 100: generic), under a tie order"""
    ambiguous = True
    thr = 0.1
    kernel = 0

    def call(self, env, batch, init, out):
        env.h.set_tie_order(self.tie)
        try:
            if self.nbest:
                return env.lib.fcd_beam_search_nbest_dev(env.h.ptr, C.byref(batch), self.beam, self.thr, 1, self.kernel,
                                                         C.byref(out.nb), C.byref(out.result))
            return env.lib.fcd_beam_search_dev(env.h.ptr, C.byref(batch), self.beam, self.thr, 1, self.kernel, C.byref(out.result))
        finally:
            env.h.set_tie_order(nat().TIE_DEFAULT)

    def reference(self, d):
        """the oracle's search (sort_unstable_by's order, the kernels' FCD_TIE_PDQ178); under FCD_TIE_STABLE it stands for the
        reads on which it counts no tie at all, and the n-best restatement's stable search for the others (16-bit
        posteriors tie now and then) -- whose tie counters are then left to the far == compact comparison"""
        import nbest_reference as NR
        stable = self.tie == nat().TIE_STABLE
        want = []
        for b in range(d["B"]):
            x = np.ascontiguousarray(d["x32"][b, :d["lengths"][b]])
            st, labels, path, n_amb = oracle.beam_search_ambiguous(x, self.beam, self.thr, True)
            if stable and n_amb != (0, 0):
                st, hyps = NR.beam_search(x, self.beam, self.thr, True, stable=True)
                labels, path, n_amb = (hyps[0][0], hyps[0][1], None) if st == 0 else ([], [], None)
            assert st == 0, (self.name, b)
            want.append((st, labels, path, n_amb))
        if self.nbest:
            d["nbest_want"] = [NR.beam_search(d["x32"][b, :d["lengths"][b]], self.beam, self.thr, True, stable=stable)
                               for b in range(d["B"])]
        return want

    def check(self, got, d):
        nb = max(self.nbest, 1)
        for b, (st, labels, path, n_amb) in enumerate(d["want"]):
            n = int(got.out_len[b * nb])
            assert int(got.status[b]) == st and n == len(labels), (self.name, b)
            assert np.array_equal(got.labels[b * nb, :n], labels), (self.name, b)
            if got.path is not None:
                assert np.array_equal(got.path[b * nb, :n], path), (self.name, b)
            if n_amb is not None:
                assert tuple(int(v) for v in got.ambiguous[b]) == n_amb, (self.name, b, got.ambiguous[b], n_amb)
        if self.nbest:
            check_nbest(got, d, self.nbest)


def check_nbest(got, d, n_best):
    import nbest_cases as NC
    B, T = d["B"], d["T"]
    r = Got()
    r.status, r.n_hyp = got.status, got.n_hyp
    r.out_len, r.score = got.out_len.reshape(B, n_best), got.score.reshape(B, n_best)
    r.labels, r.path = got.labels.reshape(B, n_best, T), got.path.reshape(B, n_best, T)
    NC.check(r, d["nbest_want"], n_best, B)


class CrfGreedy(Search):
    crf = True
    qual = True

    def call(self, env, batch, init, out):
        return env.lib.fcd_crf_greedy_search_dev(env.h.ptr, C.byref(batch), C.c_void_p(init.ptr), self.S, self.S, C.byref(out.result))

    def reference(self, d):
        return [oracle.crf_greedy_search(np.ascontiguousarray(d["x32"][b, :d["lengths"][b]]), d["init"][b], "NACGT", True)
                for b in range(d["B"])]

    def check(self, got, d):
        for b, (seq, path) in enumerate(d["want"]):
            n = int(got.out_len[b])
            assert int(got.status[b]) == 0 and n == len(path), (self.name, b)
            have = "".join("NACGT"[l] for l in got.labels[b, :n])
            if got.qual is not None:
                have += "".join(oracle.phred(float(q)) for q in got.qual[b, :n])
            else:
                seq = seq[:n]
            assert have == seq and got.path[b, :n].tolist() == path, (self.name, b)


class CrfBeam(Search):
    crf = True
    ambiguous = True
    beam = 5
    thr = 0.1

    def call(self, env, batch, init, out):
        if self.nbest:
            return env.lib.fcd_crf_beam_search_nbest_dev(env.h.ptr, C.byref(batch), C.c_void_p(init.ptr), self.S, self.S, self.beam,
                                                         self.thr, 0, C.byref(out.nb), C.byref(out.result))
        return env.lib.fcd_crf_beam_search_dev(env.h.ptr, C.byref(batch), C.c_void_p(init.ptr), self.S, self.S, self.beam, self.thr,
                                               C.byref(out.result))

    def reference(self, d):
        want = [oracle.crf_beam_search_ambiguous(np.ascontiguousarray(d["x32"][b, :d["lengths"][b]]), d["init"][b], self.beam, self.thr)
                for b in range(d["B"])]
        assert all(w[0] == 0 for w in want), self.name
        if self.nbest:
            import nbest_reference as NR
            d["nbest_want"] = [NR.crf_beam_search(d["x32"][b, :d["lengths"][b]], d["init"][b], self.beam, self.thr, stable=False)
                               for b in range(d["B"])]
        return want

    check = Beam.check


class CrfViterbi(Search):
    crf = True
    qual = True
    logp = True
    floor = True
    parks = True  # "the traceback parks emissions there" (include/fcd.h): row 0 is held to its first T entries, not to out_len

    def call(self, env, batch, init, out):
        return env.lib.fcd_crf_viterbi_search_dev(env.h.ptr, C.byref(batch), C.c_void_p(init.ptr), self.S, self.S, C.byref(out.result),
                                                  C.c_void_p(out.logp.ptr))

    def reference(self, d):
        import crf_viterbi_reference as VR
        return [VR.viterbi(d["x32"][b, :d["lengths"][b]], d["init"][b]) for b in range(d["B"])]

    def check(self, got, d):
        import crf_viterbi_cases as VC
        if got.qual is None or got.path is None:  # (the far-output runs that leave an array out: the rest of the checker)
            for b, ref in enumerate(d["want"]):
                n = int(got.out_len[b])
                assert int(got.status[b]) == ref["status"] and got.labels[b, :n].tolist() == ref["labels"], (self.name, b)
                assert VC.same_logp(float(got.logp[b]), ref["logp"]), (self.name, b)
            return
        for b, ref in enumerate(d["want"]):
            VC.check_read(got, b, ref, (self.name, b))


def searches():
    TIES = (("pdq178", 0), ("stable", 1))
    out = [Viterbi("viterbi_c%d" % c, collapse=c) for c in (0, 1)]
    out += [Beam("beam%d_%s" % (beam, tn), beam=beam, tie=tie) for beam in (5, 24, 100) for tn, tie in TIES]
    out += [CrfGreedy("crf_greedy_s%d" % S, S=S) for S in (4, 64)]
    out += [CrfBeam("crf_beam_s%d" % S, S=S) for S in (4, 64)]
    out += [CrfViterbi("crf_viterbi_s%d" % S, S=S) for S in (64, 256)]
    out += [Beam("nbest_beam5", beam=5, tie=0, nbest=4), CrfBeam("crf_nbest_s4", S=4, nbest=4)]
    # (far outputs: n_best = 2, so that the rows r * n_best + i at out_stride 2^32 + 4 stay within the memory the tests may map)
    out += [Beam("nbest2_beam5", beam=5, tie=0, nbest=2), CrfBeam("crf_nbest2_s4", S=4, nbest=2)]
    return out


SEARCHES = {s.name: s for s in searches()}

# far reads: (dtype, stride_read in elements, emulator only)
FAR_READS = [("f16", 2 ** 31 + 16, False), ("bf16", 2 ** 31 + 16, False), ("f32", 2 ** 30 + 16, False), ("f32", 2 ** 31 + 16, True),
             ("f16", 2 ** 31 + 17, False)]
FAR_ROW_STRIDE = 2 ** 25 + 8  # f16 elements; T = 70 puts rows 64 .. 69 above 2^31 elements
FAR_ROW_STRIDE_32 = 2 ** 26 + 8  # ... and above 2^32 elements, where an offset kept in 32 unsigned bits wraps (rows 32 .. above 2^31)
TS = (70, 300)
# the lattice families' far reads: (dtype, stride_read, B) -- FAR_READS with two reads, and three float16 reads 2^31 + 16 apart:
# read 2 starts above 2^32 elements (a span of 8 GiB), where an offset kept in 32 unsigned bits wraps
LATTICE_FAR_READS = [(dt, sr, 2) for dt, sr, _ in FAR_READS] + [("f16", 2 ** 31 + 16, 3)]
LATTICE_FAR_READS_GPU = [(dt, sr, 2) for dt, sr, emu_only in FAR_READS if not emu_only] + [("f16", 2 ** 31 + 16, 3)]


def far_rows_dtype(s):
    """f16, as the table says -- float32 for crf_greedy_search, whose time-major streaming kernel takes nothing else"""
    return "f32" if isinstance(s, CrfGreedy) else "f16"


def crf_T(s, T):
    """crf_viterbi_search at S = 256: the float64 restatement walks T S N cells in Python, so the long T stays with S = 64"""
    return 70 if isinstance(s, CrfViterbi) and s.S > 64 else T


def far_reads_case(env, s, dtype, stride_read, T, B=2):
    T = crf_T(s, T)
    d = s.data(B, T, dtype)
    compact = s.run(env, d)
    s.check(compact, d)
    env.reset()
    far = s.run(env, d, Layout(stride_read=stride_read))
    assert_same(far, compact, (s.name, dtype, stride_read, T))
    env.reset()
    return compact, far


def far_rows_case(env, s, B=9, T=70):
    d = s.data(B, T, far_rows_dtype(s))
    compact = s.run(env, d)
    s.check(compact, d)
    env.reset()
    far = s.run(env, d, Layout(stride_read=s.S * N, stride_t=FAR_ROW_STRIDE))
    assert_same(far, compact, (s.name, "far rows"))
    env.reset()
    return compact, far


def far_outputs_case(env, s, runs, T=70, B=2, dtype="f16"):
    """runs: (out_stride, path, qual) per far run -- one run with everything on the emulator; on the GPU labels alone at
    2^32 + 4, then path and quality at 2^30 + 4, so that no buffer passes about 4 GiB"""
    T = crf_T(s, T)
    d = s.data(B, T, dtype)
    compact = s.run(env, d)
    s.check(compact, d)
    env.reset()
    for out_stride, path, qual in runs:
        far = s.run(env, d, out_stride=out_stride, path=path, qual=qual)
        assert_same(far, compact, (s.name, "out_stride", out_stride, path, qual))
        env.reset()
    return compact


# ---- the lattice families: far labellings and far outputs (y.stride) ---------------------------------------------------
LATTICE_T = 70
FAMILIES = ("score", "align", "posterior", "edits")  # the families whose outputs y.stride addresses
ALL_FAMILIES = FAMILIES + ("occupancy",)            # ... and the one with strides of its own (fcd_occupancy)


def lattice_case(env, kind, B, n_hyp, dtype="f16", T=LATTICE_T):
    """inputs and labellings of one lattice case, built once: the labellings are what the compact viterbi_search (kind
    "ctc") or crf_greedy_search at S = 4 ("crf") returns for the reads; hypothesis 1 (n_hyp = 2) is hypothesis 0 without its
    last label"""
    key = (kind, B, n_hyp, dtype, T)
    if key in _lattice_cases:
        return _lattice_cases[key]
    s = SEARCHES["viterbi_c1" if kind == "ctc" else "crf_greedy_s4"]
    d = s.data(B, T, dtype)
    r = s.run(env, d)
    s.check(r, d)
    env.reset()
    labels, paths = np.zeros((B, n_hyp, T), np.uint8), np.zeros((B, n_hyp, T), np.uint32)
    out_len = np.zeros((B, n_hyp), np.uint32)
    for b in range(B):
        n = int(r.out_len[b])
        assert n >= 8, "the labellings are meant to have labels"
        for i in range(n_hyp):
            labels[b, i, :n - i], paths[b, i, :n - i], out_len[b, i] = r.labels[b, :n - i], r.path[b, :n - i], n - i
    c = dict(name="far_%s_b%d_h%d_%s_t%d" % (kind, B, n_hyp, dtype, T), S=s.S, N=N, T=T, B=B, n_hyp=n_hyp, dtype=dtype, xin=d["xin"],
             x32=d["x32"] if kind == "crf" else d["x32"].reshape(B, T, N), init=d["init"], lengths=d["lengths"], labels=labels,
             paths=paths, out_len=out_len, n_valid=np.full(B, n_hyp, np.uint32), collapse=True, kind=kind)
    _lattice_cases[key] = c
    return c


_lattice_cases = {}


class OccLayout:
    """where fcd_{ctc,crf}_occupancy_dev writes: the strides of fcd_occupancy in floats (None: dense rows, whole blocks one
    after the other) and the accumulate flag.  stride_row far with dense rows: whole blocks apart; stride_row = S N (or a
    little more) with stride_t far: time-major, the blocks interleaved row by row"""

    def __init__(self, stride_row=None, stride_t=None, accumulate=0):
        self.stride_row, self.stride_t, self.accumulate = stride_row, stride_t, accumulate

    def strides(self, T, SN):
        st = SN if self.stride_t is None else self.stride_t
        return (T * SN if self.stride_row is None else self.stride_row), st


ACC_FILL = np.float32(0.25)  # what the blocks hold before an accumulate = 1 call (PATTERN as a float swallows the sum)


class _OccBuffer:
    """the occ array of a call: every row the call may write prefilled (PATTERN bytes, or ACC_FILL under accumulate = 1), and
    PATTERN in a STRIP behind every block (behind the last row where the blocks interleave) and between interleaved rows"""

    def __init__(self, env, rows, T, SN, occ):
        self.rows, self.T, self.SN = rows, T, SN
        self.sr, self.st = occ.strides(T, SN)
        self.dense = self.st == SN
        assert self.dense or self.sr < self.st, "time-major: the blocks interleave row by row"
        self.reg = env.region(((rows - 1) * self.sr + (T - 1) * self.st + SN + STRIP) * 4)
        self.before = np.full(T * SN, ACC_FILL, np.float32) if occ.accumulate else np.full(T * SN * 4, PATTERN, np.uint8).view(np.float32)
        self.width = (rows - 1) * self.sr + SN  # of an interleaved row: every labelling's row t and what lies between them
        strip = np.full(STRIP * 4, PATTERN, np.uint8)
        if self.dense:
            self.guarded = [r for r in range(rows) if r == rows - 1 or self.sr >= T * SN + STRIP]
            for r in range(rows):
                self.reg.put(r * self.sr * 4, self.before)
            for r in self.guarded:
                self.reg.put((r * self.sr + T * SN) * 4, strip)
        else:
            line = np.full(self.width * 4, PATTERN, np.uint8).view(np.float32).copy()
            for r in range(rows):
                line[r * self.sr:r * self.sr + SN] = self.before[:SN]
            for t in range(T):
                self.reg.put(t * self.st * 4, line)
            self.reg.put(((T - 1) * self.st + self.width) * 4, strip)

    def read(self):
        """-> (rows, T, SN) float32; the strips and what lies between interleaved rows must be untouched"""
        rows, T, SN = self.rows, self.T, self.SN
        got = np.zeros((rows, T, SN), np.float32)
        if self.dense:
            for r in range(rows):
                got[r] = self.reg.get(r * self.sr * 4, np.float32, T * SN).reshape(T, SN)
            for r in self.guarded:
                tail = self.reg.get((r * self.sr + T * SN) * 4, np.uint8, STRIP * 4)
                assert (tail == PATTERN).all(), ("occ: written behind block", r)
        else:
            for t in range(T):
                line = self.reg.get(t * self.st * 4, np.float32, self.width)
                for r in range(rows):
                    got[r, t] = line[r * self.sr:r * self.sr + SN]
                    gap = line[r * self.sr + SN:(r + 1) * self.sr] if r + 1 < rows else line[:0]
                    assert (gap.view(np.uint8) == PATTERN).all(), ("occ: written between the rows", t, r)
            tail = self.reg.get(((T - 1) * self.st + self.width) * 4, np.uint8, STRIP * 4)
            assert (tail == PATTERN).all(), "occ: written behind the last row"
        return got


def lattice_run(env, c, family, band, y_stride=None, layout=None, occ=None):
    """one call of fcd_{ctc,crf}_<family>_dev on reads at `layout` (None: compact) with the labellings and the outputs
    addressed by y.stride at y_stride (None: compact, T) and -- family "occupancy" -- the blocks at `occ` (an OccLayout;
    None: compact) -> dict of numpy arrays shaped as the host layer returns them, entries beyond a labelling 0; occupancy:
    "occ" with all T rows of every block as the call left them, "before" what they held"""
    n = nat()
    B, n_hyp, T = c["B"], c["n_hyp"], c["T"]
    rows, W = B * n_hyp, (T if y_stride is None else y_stride)
    batch, keep = place_batch(env, c["xin"], layout or Layout(), c["dtype"], c["lengths"], c["S"])
    init = env.small(c["init"]) if c["kind"] == "crf" else None
    # the arrays addressed with y.stride: (name, dtype, elements per unit of stride, extra units)
    arrays = [("labels", np.uint8, 1, 0)] + ([("path", np.uint32, 1, 0)] if band else [])
    arrays += {"score": [], "align": [("start", np.uint32, 1, 0), ("count", np.uint32, 1, 0), ("qual", np.float32, 1, 0)],
               "posterior": [("post", np.float32, N - 1, 0)],
               "edits": [("deletion", np.float32, 1, 0), ("insertion", np.float32, N - 1, 1)], "occupancy": []}[family]
    subs = {}
    if y_stride is None:
        for name, dt, per, extra in arrays:
            subs[name] = env.region(rows * (W + extra) * per * np.dtype(dt).itemsize)
    else:
        assert rows == 2, "a far lattice layout holds two rows"
        widest = max((W + extra) * per * np.dtype(dt).itemsize for name, dt, per, extra in arrays)
        span = env.region(widest + SLOT * (len(arrays) + 1))
        for k, (name, dt, per, extra) in enumerate(arrays):
            subs[name] = _Sub(span, k * SLOT)
    step = {name: (W + extra) * per * np.dtype(dt).itemsize for name, dt, per, extra in arrays}
    for r in range(rows):
        b, i = divmod(r, n_hyp)
        subs["labels"].put(r * step["labels"], c["labels"][b, i])
        if band:
            subs["path"].put(r * step["path"], c["paths"][b, i])
        for name, dt, per, extra in arrays[2 if band else 1:]:
            subs[name].put(r * step[name], np.full((T + extra) * per * np.dtype(dt).itemsize, PATTERN, np.uint8))
    lens, nv = env.small(c["out_len"]), env.small(c["n_valid"])
    logp = env.small(np.full(rows, 7.0))
    if family == "occupancy":
        occ = occ or OccLayout()
        ob = _OccBuffer(env, rows, T, c["S"] * N, occ)
    y = n.Labellings(subs["labels"].ptr, lens.ptr, nv.ptr, subs["path"].ptr if band else None, n_hyp, W)
    out = {"score": C.c_void_p(logp.ptr),
           "align": lambda: n.Alignment(subs["start"].ptr, subs["count"].ptr, subs["qual"].ptr, logp.ptr),
           "posterior": lambda: n.Posterior(subs["post"].ptr, logp.ptr),
           "edits": lambda: n.Edits(subs["deletion"].ptr, subs["insertion"].ptr, logp.ptr),
           "occupancy": lambda: n.Occupancy(ob.reg.ptr, ob.sr, ob.st, 1.0, occ.accumulate, logp.ptr)}[family]
    out = out if family == "score" else C.byref(out())
    fn = getattr(env.lib, "fcd_%s_%s_dev" % (c["kind"], family))
    if c["kind"] == "ctc":
        rc = fn(env.h.ptr, C.byref(batch), C.byref(y), 1, band, out)
    else:
        rc = fn(env.h.ptr, C.byref(batch), C.c_void_p(init.ptr), c["S"], c["S"], C.byref(y), band, out)
    assert rc != n.E_UNSUPPORTED, (c["name"], family, band, W, env.lib.fcd_last_error(env.h.ptr))
    assert rc == n.OK, (c["name"], family, band, W, rc, env.lib.fcd_last_error(env.h.ptr))
    env.sync()
    got = dict(logp=logp.get(0, np.float64, rows).reshape(B, n_hyp))
    for name, dt, per, extra in arrays[2 if band else 1:]:
        a = np.zeros((rows, (T + extra) * per), dt)
        for r in range(rows):
            b, i = divmod(r, n_hyp)
            L = int(c["out_len"][b, i])
            a[r, :(L + extra) * per] = subs[name].get(r * step[name], dt, (L + extra) * per)
        got[name] = a.reshape((B, n_hyp, T + extra) + ((per,) if per > 1 else ()))
    if family == "occupancy":
        shape = (B, n_hyp, T) + ((c["S"], N) if c["kind"] == "crf" else (N,))
        got["occ"] = ob.read().reshape(shape)
        got["before"] = np.broadcast_to(ob.before.reshape(shape[2:]), shape).copy()
    del keep
    return got


def occupancy_refs(c, band):
    """the float64 occupancies of the case's labellings (tests/{ctc,crf}_occupancy_reference.py), computed once per band"""
    refs = c.setdefault("occ_refs", {})
    if band not in refs:
        O = __import__("%s_occupancy_reference" % c["kind"])
        refs[band] = {}
        for b in range(c["B"]):
            Tr = int(c["lengths"][b])
            for i in range(c["n_hyp"]):
                L = int(c["out_len"][b, i])
                y, path = c["labels"][b, i, :L], (c["paths"][b, i, :L] if band else None)
                refs[band][(b, i)] = (O.occupancy64(c["x32"][b, :Tr], c["init"][b], y, band, path) if c["kind"] == "crf" else
                                      O.occupancy64(c["x32"][b, :Tr], y, True, band, path))
    return refs[band]


def occupancy_check(got, c, band, accumulate, score):
    """the table's case dict as tests/{ctc,crf}_occupancy_cases.py's check takes it: that checker, its bounds, its rules on
    what stays untouched; score: the logp of the score family on the same case (the same bits)"""
    M = __import__("%s_occupancy_cases" % c["kind"])
    cc = dict(c, band=band, refs=occupancy_refs(c, band), accumulate=bool(accumulate))
    if c["kind"] == "ctc":
        cc["k"] = M.states_per_lane(c["T"], c["T"], band)  # (the labellings are compact here: y.stride = T)
    M.check(cc, got["occ"], got["logp"], score, got["before"])


def lattice_check(got, c, family, band, accumulate=0, score=None):
    """the compact result against the family's restatement, with the family's own checker and bounds"""
    from fast_ctc_decode_amd import api
    kind = c["kind"]
    args = (c["lengths"], c["labels"], c["paths"], c["out_len"], c["n_valid"])
    if family == "occupancy":
        occupancy_check(got, c, band, accumulate, score)
    elif family in ("score", "align") and kind == "crf":
        import crf_lattice_cases as CC
        if family == "score":  # (CC.check takes the alignment too: the score alone against the restatement here)
            import crf_lattice_reference as R
            for b in range(c["B"]):
                Tr = int(c["lengths"][b])
                for i in range(c["n_hyp"]):
                    L = int(c["out_len"][b, i])
                    want = R.crf_score(c["x32"][b, :Tr], c["init"][b], c["labels"][b, i, :L], band, c["paths"][b, i, :L] if band else None)
                    assert abs(got["logp"][b, i] - want) <= CC.tolerance(Tr), (c["name"], band, b, i, got["logp"][b, i], want)
        else:
            CC.check(api.AlignResult(got["start"], got["count"], got["qual"], got["logp"]), None, c["x32"], c["init"], *args, band)
    elif family == "score":
        import ctc_score_cases as SC
        SC.check(got["logp"], c["x32"], *args, True, band)
    elif family == "align":
        import ctc_align_cases as AC
        AC.check(api.AlignResult(got["start"], got["count"], got["qual"], got["logp"]), c["x32"], *args, True, band)
    elif family == "posterior":
        M = __import__("crf_posterior_cases" if kind == "crf" else "ctc_posterior_cases")
        res = api.PosteriorResult(got["post"], got["logp"])
        M.check(res, c, band) if kind == "crf" else M.check(res, c, band, verbose=False)
    else:
        M = __import__("crf_edits_cases" if kind == "crf" else "ctc_edits_cases")
        res = api.EditResult(got["deletion"], got["insertion"], got["logp"])
        M.check(res, c, band) if kind == "crf" else M.check(res, c, band, verbose=False)


def lattice_far_case(env, kind, family, band, B, n_hyp, y_stride=None, T=LATTICE_T, layout=None, dtype="f16", occ=None, launched=None,
                     c=None):
    """compact against the restatement, far == compact bit for bit, and a workspace that does not grow with a stride.  ONE
    of y_stride (labellings and the outputs they address), layout (the reads) and occ (an OccLayout: the occupancy blocks) is
    far.  launched: the emulator runner's look at the launch log -- the far call launches what the compact call did.
    -> the far result"""
    c = c or lattice_case(env, kind, B, n_hyp, dtype, T)
    where = (c["name"], family, band, y_stride, layout and layout.strides(T, c["S"] * N), occ and (occ.strides(T, c["S"] * N), occ.accumulate))
    accumulate = occ.accumulate if occ else 0
    score = None
    if family == "occupancy":  # (logp must be the score family's bits on the same case)
        score = lattice_run(env, c, "score", band)["logp"]
        env.reset()
    env.h.release_workspace()
    if launched:
        launched()
    compact = lattice_run(env, c, family, band, occ=OccLayout(accumulate=accumulate))
    ws_compact = env.workspace_bytes()
    lattice_check(compact, c, family, band, accumulate, score)
    env.reset()
    ran = launched() if launched else None
    far = lattice_run(env, c, family, band, y_stride, layout, occ)
    ws_far = env.workspace_bytes()
    env.reset()
    if launched:
        ran_far = launched()
        assert ran_far == ran, (where, "the far call launched other instantiations", sorted(ran ^ ran_far))
    for name in compact:
        assert np.array_equal(bits(far[name]), bits(compact[name])), (where, name)
    assert ws_far == ws_compact, (where, "the workspace grew with a stride", ws_compact, ws_far)
    return far


# ---- the occupancy blocks (fcd_occupancy.stride_row / stride_t) ----------------------------------------------------------
OCC_FAR_ROW = 2 ** 31 + 4  # floats between two dense blocks: block 1 above 2^31 elements (8 GiB)
# time-major, T = 70: rows 64 .. 69 of both labellings above 2^31 elements; (stride_row extra, ...) once dense, once padded
OCC_FAR_T = FAR_ROW_STRIDE


def occupancy_grouped_case(env, kind, band, stride_row=OCC_FAR_ROW):
    """a workspace limit of one byte: every read is a launch group of its own and the host adds row0 * stride_row to the base
    -- the same bits as the far call in one group"""
    c = lattice_case(env, kind, 2, 1)
    occ = OccLayout(stride_row=stride_row)
    whole = lattice_far_case(env, kind, "occupancy", band, 2, 1, occ=occ)
    env.h.set_workspace_limit(1)
    try:
        parts = lattice_run(env, c, "occupancy", band, occ=occ)
    finally:
        env.h.set_workspace_limit(0)
        env.reset()
    for name in whole:
        assert np.array_equal(bits(parts[name]), bits(whole[name])), (c["name"], band, "one read per group", name)


def occupancy_no_value_case(env, kind, accumulate, stride_row=OCC_FAR_ROW):
    """the labelling at the far block has more labels than its read has rows: P(y | x) = 0, logp = -inf, and nothing of its
    block is written, in either accumulate mode"""
    key = (kind, "more labels than rows")
    if key not in _lattice_cases:
        c = dict(lattice_case(env, kind, 2, 1))
        Tr = int(c["lengths"][1])
        assert Tr + 1 <= c["T"]
        c["labels"], c["out_len"] = c["labels"].copy(), c["out_len"].copy()
        c["labels"][1, 0, :Tr + 1] = np.random.default_rng(5).integers(1, N, Tr + 1)
        c["out_len"][1, 0] = Tr + 1
        c["name"] += "_long"
        c.pop("occ_refs", None)
        _lattice_cases[key] = c
    c = _lattice_cases[key]
    far = lattice_far_case(env, kind, "occupancy", 0, 2, 1, occ=OccLayout(stride_row=stride_row, accumulate=accumulate), c=c)
    assert occupancy_refs(c, 0)[(1, 0)]["occ"] is None and far["logp"][1, 0] == -np.inf
    assert np.array_equal(bits(far["occ"][1]), bits(far["before"][1])), "the block of a labelling without a value was written"
    assert np.isfinite(far["logp"][0, 0])


# ---- the walks over all labellings: fcd_crf_transition_probs_dev and fcd_crf_marginals_dev -------------------------------
# one shape per code form (tests/instantiation_cases.py): a lane per element (S N <= 64), one chunk of 64 states, many chunks
WALK_SHAPES = ((4, 7), (64, 9), (256, 7))
WALK_AXES = ("scores_read", "scores_t", "out_read", "out_t", "init", "emit")


def walk_case(which, S, T, dtype="f32", layout="source", out="f32"):
    """a case of tests/crf_transitions_cases.py / crf_marginals_cases.py (inputs and references built once there), of which
    the table runs reads 0 and 1: lengths T and T - 3"""
    import crf_marginals_cases as MC
    import crf_transitions_cases as TC
    case = TC._case("far_s%d_t%d_%s_%s_%s" % (S, T, dtype, layout, out), S, N, T, dtype=dtype, layout=layout, out=out)
    if which == "marginals":
        case = dict(case, name="m_" + case["name"])
        return MC.build_case(case)
    return TC.build_case(case)


def _rows(reg, B, T, sr, st, inner, dtype):
    """(B, T, inner) read back from a region at the strides sr, st (elements)"""
    e = np.dtype(dtype).itemsize
    got = np.zeros((B, T, inner), dtype)
    if st == inner:
        for b in range(B):
            got[b] = reg.get(b * sr * e, dtype, T * inner).reshape(T, inner)
    else:
        assert sr == inner, "time-major"
        for t in range(T):
            got[:, t] = reg.get(t * st * e, dtype, B * inner).reshape(B, inner)
    return got


def walk_run(env, which, c, axis=None, stride=None):
    """one call of fcd_crf_transition_probs_dev / fcd_crf_marginals_dev on reads 0 and 1 of the case with ONE quantity at
    `stride` (elements): axis "scores_read" / "scores_t" (time-major) the input, "out_read" / "out_t" (time-major) probs or
    marg, "init" init_stride, "emit" emit_stride; None: everything compact.  Every output row is PATTERN beforehand, with a
    STRIP behind the last; the scores must be what they were.  -> dict of numpy arrays, all T rows of every read"""
    n = nat()
    B, T, S = 2, c["T"], c["S"]
    SN = S * N
    marg = which == "marginals"
    assert axis is None or axis in WALK_AXES and not (axis == "init" and marg) and not (axis == "emit" and not marg)
    xin, lengths = c["xin"][:B], c["lengths"][:B]
    lay = Layout(stride_read=stride) if axis == "scores_read" else Layout(stride_read=SN, stride_t=stride) if axis == "scores_t" else Layout()
    batch, keep = place_batch(env, xin, lay, c["dtype"], lengths, S)
    in_sr, in_st = lay.strides(T, SN)
    odt = np.float16 if c["out"] == "f16" else np.float32
    e = np.dtype(odt).itemsize
    sr, st = (stride, SN) if axis == "out_read" else (SN, stride) if axis == "out_t" else (T * SN, SN)

    def filled(count, row, step, esz):
        """a region of `count` rows of `row` elements `step` apart: PATTERN in every row and in a STRIP behind the last"""
        reg = env.region(((count - 1) * step + row + STRIP) * esz)
        for k in range(count):
            reg.fill(k * step * esz, (row + (STRIP if k == count - 1 else 0)) * esz)
        return reg
    if st == SN:
        main = filled(B, T * SN, sr, e)
    else:
        main = filled(T, B * SN, st, e)
    init_stride = stride if axis == "init" else S
    emit_stride = stride if axis == "emit" else T * N
    init = None if marg else filled(B, S, init_stride, 4)
    emit = filled(B, T * N, emit_stride, 4) if marg else None
    logz, status = env.small(np.full(B, 7.0)), env.small(np.full(B, -7, np.int32))
    lcode = n.LAYOUT_DEST if c["layout"] == "dest" else n.LAYOUT_SOURCE
    if marg:
        out = n.Marginals(main.ptr, sr, st, emit.ptr, emit_stride, logz.ptr, status.ptr)
        rc = env.lib.fcd_crf_marginals_dev(env.h.ptr, C.byref(batch), lcode, C.byref(out))
    else:
        out = n.Transitions(main.ptr, n.DTYPE_F16 if c["out"] == "f16" else n.DTYPE_F32, sr, st, init.ptr, init_stride, logz.ptr, status.ptr)
        rc = env.lib.fcd_crf_transition_probs_dev(env.h.ptr, C.byref(batch), lcode, C.byref(out))
    assert rc == n.OK, (which, c["name"], axis, stride, rc, env.lib.fcd_last_error(env.h.ptr))
    env.sync()
    got = dict(main=_rows(main, B, T, sr, st, SN, odt).reshape(B, T, S, N), logz=logz.get(0, np.float64, B), status=status.get(0, np.int32, B))
    last = ((B - 1) * sr + T * SN) if st == SN else ((T - 1) * st + B * SN)
    assert (main.get(last * e, np.uint8, STRIP * e) == PATTERN).all(), (which, c["name"], axis, "written behind the last row")
    for name, reg, row, step in (("init", init, S, init_stride), ("emit", emit, T * N, emit_stride)):
        if reg is not None:
            got[name] = np.stack([reg.get(b * step * 4, np.float32, row) for b in range(B)])
            assert (reg.get(((B - 1) * step + row) * 4, np.uint8, STRIP * 4) == PATTERN).all(), (which, c["name"], axis, name, "written behind the last row")
    if marg:
        got["emit"] = got["emit"].reshape(B, T, N)
    back = _rows(keep[0], B, T, in_sr, in_st, SN, xin.dtype)
    assert np.array_equal(back, xin.reshape(B, T, SN)), (which, c["name"], axis, "the scores were written")
    for b in range(B):  # rows t >= T_r are not written
        for name in ("main", "emit") if marg else ("main",):
            assert (np.ascontiguousarray(got[name][b, int(lengths[b]):]).view(np.uint8) == PATTERN).all(), (which, c["name"], axis, name, b)
    del keep
    return got


def walk_check(which, c, got):
    """the compact result against the float64 restatement: check_read of tests/crf_transitions_cases.py /
    crf_marginals_cases.py with its bounds (it wants its own sentinel in the rows t >= T_r, which walk_run found untouched)"""
    import crf_marginals_cases as MC
    import crf_transitions_cases as TC
    for b in range(2):
        Tr = int(c["lengths"][b])
        main = got["main"][b].copy()
        main[Tr:] = TC.SENTINEL
        if which == "marginals":
            emit = got["emit"][b].copy()
            emit[Tr:] = TC.SENTINEL
            MC.check_read(c, b, main, emit, float(got["logz"][b]), got["status"][b], (c["name"], b))
        else:
            TC.check_read(c, b, main, got["init"][b], float(got["logz"][b]), got["status"][b], (c["name"], b))


def walk_far_case(env, which, S, T, axis, stride, dtype="f32", layout="source", out="f32", launched=None):
    """compact against the restatement; far == compact bit for bit on every row t < T_r, init / emit, logz and status; no
    workspace either way"""
    c = walk_case(which, S, T, dtype, layout, out)
    env.h.release_workspace()
    if launched:
        launched()
    compact = walk_run(env, which, c)
    walk_check(which, c, compact)
    env.reset()
    ran = launched() if launched else None
    far = walk_run(env, which, c, axis, stride)
    ws = env.workspace_bytes()
    env.reset()
    where = (which, c["name"], axis, stride)
    if launched:
        ran_far = launched()
        assert ran_far == ran, (where, "the far call launched other instantiations", sorted(ran ^ ran_far))
    assert ws == 0, (where, "the walks take no workspace", ws)
    for name in compact:
        for b in range(2):
            rows = slice(0, int(c["lengths"][b])) if name in ("main", "emit") else Ellipsis  # (rows t >= T_r: found untouched)
            assert np.array_equal(bits(np.atleast_1d(far[name][b])[rows]), bits(np.atleast_1d(compact[name][b])[rows])), (where, name, b)
    return far


def walk_row_stride(T, esize, elements=True):
    """the stride_t of a time-major far-rows case: T = 70 takes FAR_ROW_STRIDE for float32 rows (rows 64 .. 69 above 2^31
    elements) and FAR_ROW_STRIDE_32 for two-byte rows; the short T of S = 256 a stride that puts rows T // 2 and up above 2^31
    elements, or -- elements False: where that span does not fit the GPU's pool -- above 2^32 bytes"""
    if T >= 70:  # (two-byte elements: rows 64 .. 69 above 2^32 elements as well, in the same 8.63 GiB)
        return FAR_ROW_STRIDE_32 if esize == 2 else FAR_ROW_STRIDE
    boundary = 2 ** 31 if elements else 2 ** 32 // esize
    return -(-boundary // (T // 2)) // 8 * 8 + 8


def walk_table(gpu):
    """(which, S, T, axis, stride, dtype, layout, out) of every far case of the two walks.  Each axis is far alone.  gpu: the
    strides whose span fits the GPU runner's pool -- bytes past 2^32 where elements past 2^31 do not fit"""
    rows = []
    for which in ("transitions", "marginals"):
        outs = ("f32", "f16") if which == "transitions" else ("f32",)
        for S, T in WALK_SHAPES:
            for dtype, stride, emu_only in (("f16", 2 ** 31 + 16, False), ("f32", 2 ** 30 + 16, False), ("f32", 2 ** 31 + 16, True)):
                if not (gpu and emu_only):
                    rows += [(which, S, T, "scores_read", stride, dtype, lay, "f32") for lay in ("source", "dest")]
            Tt = T if S > 64 else 70  # (far rows: T = 70, S = 256 at its short T)
            rows += [(which, S, Tt, "scores_t", walk_row_stride(Tt, 2), "f16", lay, "f32") for lay in ("source", "dest")]
            for out in outs:
                e = 2 if out == "f16" else 4
                rows.append((which, S, T, "out_read", 2 ** 31 + 4, "f32", "source", out))
                rows.append((which, S, Tt, "out_t", walk_row_stride(Tt, e, not (gpu and e == 4)), "f32", "source", out))
            rows.append((which, S, T, "init" if which == "transitions" else "emit", 2 ** 31 + 4, "f32", "source", "f32"))
    return rows


def walk_id(row):
    return "%s-s%d-t%d-%s-%d-%s-%s-%s" % row


# ---- pack / offsets / unpack of a far result -------------------------------------------------------------------------
def pack_case(env, out_stride, T=70):
    """viterbi_search into a result at out_stride, fcd_result_offsets_dev / fcd_pack_results_dev on it, fcd_unpack_results_dev
    into a compact result and into another far one: both equal the compact search (which equals the oracle)"""
    n = nat()
    s = SEARCHES["viterbi_c1"]
    B = 2
    d = s.data(B, T, "f16")
    compact = s.run(env, d)
    s.check(compact, d)
    env.reset()
    far, out = s.run(env, d, out_stride=out_stride, qual=False, keep_out=True)
    assert_same(far, compact, ("pack", out_stride, "the search"))
    offs = env.small(np.full(B + 1, 0x7777, np.uint64))
    env.h.check(env.lib.fcd_result_offsets_dev(env.h.ptr, out.out_len.ptr, B, out_stride, offs.ptr))
    env.sync()
    want_offs = np.concatenate([[0], np.cumsum(compact.out_len.astype(np.uint64))]).astype(np.uint64)
    assert np.array_equal(offs.get(0, np.uint64, B + 1), want_offs)
    total = int(want_offs[B])
    path_bytes = 2 if out_stride <= 65535 else 4  # (fast_ctc_decode_amd/dist.py: the width switch of the wire format)
    nbytes = int(env.lib.fcd_packed_result_bytes(B, total, path_bytes))
    buf = env.region(nbytes + 16)
    env.h.check(env.lib.fcd_pack_results_dev(env.h.ptr, C.byref(out.result), B, path_bytes, offs.ptr, buf.ptr))
    for W in (None, out_stride):
        back = Out(env, B, T, W, True, False)
        work = env.small(np.zeros(B + 1, np.uint64))
        env.h.check(env.lib.fcd_unpack_results_dev(env.h.ptr, buf.ptr, B, work.ptr, C.byref(back.result)))
        assert_same(back.read(), compact, ("pack", out_stride, "unpacked at", W))
    env.reset()


# ---- an arena above 4 GiB (GPU only) ---------------------------------------------------------------------------------
ARENA_B = 512
ARENA_RANGE = (4.5 * 2 ** 30, 7.0 * 2 ** 30)


def arena_bytes(kernel, T, B, beam):
    """the worst-case tree arena of one fcd_beam_search_dev launch at N = 5, as csrc/capi.hip sizes it (run_beam): a slab
    per read of cap_nodes nodes -- records, jump pointers and child rows for the register kernels (plus the lane kernel's
    table of first ids), int4 records and N - 1 child words for the LDS-resident kernel"""
    NL = N - 1
    if kernel == "wave":
        cap = ((T << 5) + 8 + 3) & ~3          # one block of 1 << 5 ids per step at beam <= 5, N <= 5
        return cap * (4 + 4 + 4 * 4) * B
    if kernel == "lane":
        cap = (T * min(beam, 64) * NL + 8 + 3) & ~3
        return (cap * (4 + 4 + 4 * 4) + ((T + 1 + 3) & ~3) * 4) * B
    return (T * beam * NL + 8) * (16 + 4 * NL) * B


def arena_T(kernel, beam, B=ARENA_B, at_least=ARENA_RANGE[0]):
    """the smallest T whose arena reaches the range with B reads"""
    T = 1
    while arena_bytes(kernel, T, B, beam) < at_least:
        T += 1
    return T


def arena_case(env, kernel, beam, B=ARENA_B, bounds=ARENA_RANGE, overlap=0):
    """ONE launch whose arena lies between 4.5 and 7 GiB, a slab per read: the last reads' slabs start above 2^32 bytes
    from the arena's base.  The first four and the last eight reads against the oracle; every read against the same reads
    decoded eight at a time (arenas of a few MiB: the regime the rest of the suite pins to the oracle).  overlap: the
    eight-read calls go round-robin to that many internal streams (fcd_set_overlap) -- the LDS-resident kernel takes a
    tenth of a second per call here, one read a block, and 64 of them in stream order would take the test past its seconds.
    -> (T, arena bytes by the formula, the handle's workspace after the launch)"""
    n = nat()
    T = arena_T(kernel, beam, B, bounds[0])
    want_bytes = arena_bytes(kernel, T, B, beam)
    assert bounds[0] <= want_bytes <= bounds[1], (kernel, T, want_bytes)
    if bounds is ARENA_RANGE:
        assert arena_bytes(kernel, T, B - 8, beam) > 2 ** 32, "the last eight reads' slabs start above 2^32 bytes"
    rng = np.random.default_rng(600 + beam)
    x = rng.random((B, T, N), dtype=np.float32) ** 3
    x /= np.linalg.norm(x, axis=2, keepdims=True)
    xin, x32 = to_dtype(x, "f16")
    lengths = ragged(B, T)
    s = Beam("arena_%s" % kernel, beam=beam, tie=n.TIE_PDQ178, thr=0.05, ambiguous=False,
             kernel={"wave": n.KERNEL_WAVE, "lane": n.KERNEL_LANE, "generic": n.KERNEL_GENERIC}[kernel])
    e = ESIZE["f16"]
    batch, keep = place_batch(env, xin, Layout(), "f16", lengths)
    env.h.release_workspace()
    try:
        return _arena_launches(env, s, batch, kernel, beam, B, T, x32, lengths, want_bytes, overlap)
    finally:  # the handle is shared: stream order, and the arena given back
        env.sync()
        env.h.set_overlap(0)
        env.h.release_workspace()
        del keep


def _arena_launches(env, s, batch, kernel, beam, B, T, x32, lengths, want_bytes, overlap):
    n, e = nat(), ESIZE["f16"]
    parts = []
    env.h.set_overlap(overlap)
    for r0 in range(0, B, 8):  # eight at a time, on views of the same device array
        sub = n.Batch(batch.post + r0 * T * N * e, 8, T, 1, N, T * N, N, 0, 1, batch.lengths + r0 * 8, DTYPE_CODE["f16"])
        out = Out(env, 8, T)
        assert s.call(env, sub, None, out) == n.OK, env.lib.fcd_last_error(env.h.ptr)
        parts.append(out)
    parts = [o.read() for o in parts]
    env.h.set_overlap(0)
    assert env.workspace_bytes() <= 2 * want_bytes * 8 * max(overlap, 1) // B, "eight reads at a time: a small arena"
    out = Out(env, B, T)
    assert s.call(env, batch, None, out) == n.OK, env.lib.fcd_last_error(env.h.ptr)
    whole = out.read()
    ws = env.workspace_bytes()
    assert ws >= want_bytes, ("the launch was chunked: the arena is smaller than one slab per read", ws, want_bytes)
    for b in list(range(4)) + list(range(B - 8, B)):
        st, labels, path, _ = oracle.beam_search_raw(np.ascontiguousarray(x32[b, :lengths[b]]), beam, s.thr, True)
        k = int(whole.out_len[b])
        assert st == 0 and int(whole.status[b]) == 0 and k == len(labels), (kernel, b)
        assert np.array_equal(whole.labels[b, :k], labels) and np.array_equal(whole.path[b, :k], path), (kernel, b)
    for i, part in enumerate(parts):
        sl = slice(8 * i, 8 * i + 8)
        assert np.array_equal(whole.status[sl], part.status) and np.array_equal(whole.out_len[sl], part.out_len), (kernel, i)
        for j in range(8):
            k = int(part.out_len[j])
            assert np.array_equal(whole.labels[8 * i + j, :k], part.labels[j, :k]), (kernel, 8 * i + j)
            assert np.array_equal(whole.path[8 * i + j, :k], part.path[j, :k]), (kernel, 8 * i + j)
    return T, want_bytes, ws


# the lattice families at T = 300, one labelling per read: (kind, family, band).  Exact mode stops at 254 labels for
# ctc_posterior / ctc_edits (include/fcd.h: "use a band"), and the float64 restatement of crf_posterior / crf_edits rescoring
# every variant of 150 labels exactly takes several seconds -- those four run with the band alone
LATTICE_300 = [(kind, fam, band) for kind in ("ctc", "crf") for fam in FAMILIES for band in (0, 6)
               if not (band == 0 and fam in ("posterior", "edits"))]
# the duplex layouts: (dtype, stride_read or None for far rows, T1)
DUPLEX_LAYOUTS = [("f16", 2 ** 31 + 16, 70), ("f32", 2 ** 30 + 16, 70), ("f16", 2 ** 31 + 17, 70), ("f16", None, 70),
                  ("f16", 2 ** 31 + 16, 300)]


# ---- a session pushed in two chunks from a far buffer ------------------------------------------------------------------
def session_case(env, dtype, stride_read, T=70, cut=40):
    """fcd_beam_session_push_dev twice (rows [0, cut) and [cut, T), ragged) from reads stride_read apart: the result after
    the second push is beam_search's on the whole reads -- the oracle's -- from the compact buffer and from the far one"""
    n = nat()
    s = SEARCHES["beam5_pdq178"]
    B = 2
    d = s.data(B, T, dtype)
    e, got = ESIZE[dtype], []
    for layout in (Layout(), Layout(stride_read=stride_read)):
        batch, keep = place_batch(env, d["xin"], layout, dtype, d["lengths"])
        ses = C.c_void_p()
        env.h.check(env.lib.fcd_beam_session_create(env.h.ptr, B, N, T, s.beam, s.thr, 1, n.KERNEL_AUTO, 0, C.byref(ses)))
        try:
            for r0, r1 in ((0, cut), (cut, T)):
                rows = np.clip(d["lengths"] - r0, 0, r1 - r0).astype(np.int64)  # (a HOST array: include/fcd.h, push)
                chunk = n.Batch(batch.post + r0 * batch.stride_t * e, B, r1 - r0, 1, N, batch.stride_read, batch.stride_t, 0, 1,
                                rows.ctypes.data, DTYPE_CODE[dtype])
                rc = env.lib.fcd_beam_session_push_dev(ses, C.byref(chunk), None)
                assert rc == n.OK, (rc, env.lib.fcd_last_error(env.h.ptr))
            out = Out(env, B, T)
            rc = env.lib.fcd_beam_session_result_dev(ses, C.byref(out.result))
            assert rc == n.OK, (rc, env.lib.fcd_last_error(env.h.ptr))
            got.append(out.read())
        finally:
            env.sync()
            assert env.lib.fcd_beam_session_destroy(ses) == n.OK
        del keep
        env.reset()
    for b, (st, labels, path, _) in enumerate(d["want"]):
        k = int(got[0].out_len[b])
        assert int(got[0].status[b]) == st and k == len(labels), ("session", b)
        assert np.array_equal(got[0].labels[b, :k], labels) and np.array_equal(got[0].path[b, :k], path), ("session", b)
    assert_same(got[1], got[0], ("session", dtype, stride_read), fields=("labels", "path"))


# ---- the duplex searches with both batches far, and the band estimator -------------------------------------------------
ALPHA = "NACGT"


def _duplex_data(crf, dtype, T1=70):
    key = (crf, dtype, T1)
    if key not in _duplex:
        import test_gpu_duplex as D
        B, T2 = 2, T1 - 4
        if crf:
            ps = [D.crf_pairs(7300 + T1 + i, T1, T2) for i in range(B)]
            x1, x2 = np.stack([p[0] for p in ps]), np.stack([p[2] for p in ps])
            i1, i2 = np.stack([p[1] for p in ps]), np.stack([p[3] for p in ps])
        else:
            (x1, x2), i1, i2 = D.pairs(7200 + T1, B, T1, T2), None, None
        (q1, up1), (q2, up2) = to_dtype(x1, dtype), to_dtype(x2, dtype)
        l1, l2 = ragged(B, T1), ragged(B, T2)
        env = np.zeros((B, T1, 2), np.uint64)
        for i in range(B):
            env[i, :l1[i]] = D.band(int(l1[i]), int(l2[i]), 12)
        _duplex[key] = dict(q1=q1, q2=q2, up1=up1, up2=up2, i1=i1, i2=i2, l1=l1, l2=l2, env=env, B=B, T1=T1, T2=T2, want={})
    return _duplex[key]


_duplex = {}


def duplex_case(env, crf, which, mode, dtype, stride_read=None, T1=70):
    """fcd_beam_search_duplex_dev / fcd_crf_beam_search_duplex_dev on the kernel `which` (fcd_debug_set_duplex_kernel: 1 the
    any-shape kernel, 2 the slot-resident one) with BOTH batches far: their reads stride_read apart, or -- stride_read None
    -- time-major with the ROWS FAR_ROW_STRIDE apart (stride_read = S N; T1 = 70, T2 = 66: rows 64 and up lie above 2^31
    elements in both).  mode: 0 logsumexp, 1 max"""
    import test_gpu_duplex as D
    n = nat()
    d = _duplex_data(crf, dtype, T1)
    B, T1, S = d["B"], d["T1"], 4 if crf else 1
    omode = (D.MAX if mode else D.LSE) | D.CR
    if mode not in d["want"]:
        want = []
        for i in range(B):
            a, b, ev = d["up1"][i, :d["l1"][i]], d["up2"][i, :d["l2"][i]], d["env"][i, :d["l1"][i]]
            if crf:
                want.append(oracle.crf_beam_search_duplex(a, d["i1"][i], b, d["i2"][i], ALPHA, ev, 5, 0.05, omode))
            else:
                want.append(oracle.beam_search_duplex(a, b, ALPHA, ev, 5, 0.05, True, omode))
        assert all(len(w) > 0 for w in want)
        d["want"][mode] = want
    got = []
    assert env.lib.fcd_debug_set_duplex_kernel(env.h.ptr, which) == n.OK
    try:
        far = Layout(stride_read=stride_read) if stride_read else Layout(stride_read=S * N, stride_t=FAR_ROW_STRIDE)
        for layout in (Layout(), far):
            b1, k1 = place_batch(env, d["q1"], layout, dtype, d["l1"], S)
            b2, k2 = place_batch(env, d["q2"], layout, dtype, d["l2"], S)
            ev = env.small(d["env"])
            out = Out(env, B, T1, path=False)
            if crf:
                i1, i2 = env.small(d["i1"]), env.small(d["i2"])
                rc = env.lib.fcd_crf_beam_search_duplex_dev(env.h.ptr, C.byref(b1), C.c_void_p(i1.ptr), S, S, C.byref(b2), C.c_void_p(i2.ptr),
                                                            S, S, C.c_void_p(ev.ptr), T1, 5, 0.05, mode, C.byref(out.result))
            else:
                rc = env.lib.fcd_beam_search_duplex_dev(env.h.ptr, C.byref(b1), C.byref(b2), C.c_void_p(ev.ptr), T1, 5, 0.05, 1, mode,
                                                        C.byref(out.result))
            assert rc == n.OK, (rc, env.lib.fcd_last_error(env.h.ptr))
            got.append(out.read())
            del k1, k2
            env.reset()
    finally:
        assert env.lib.fcd_debug_set_duplex_kernel(env.h.ptr, 0) == n.OK
    for i, w in enumerate(d["want"][mode]):
        k = int(got[0].out_len[i])
        assert int(got[0].status[i]) == 0, (crf, which, mode, i)
        lab = got[0].labels[i, :k]
        have = "".join(ALPHA[l] for l in lab[::-1])[::-1] if crf else "".join(ALPHA[l] for l in lab)  # (src/duplex.rs:825-833)
        assert have == w, (crf, which, mode, i, have, w)
    assert_same(got[1], got[0], ("duplex", crf, which, mode, dtype, stride_read, T1), fields=("labels",))


def envelope_case(env, stride, env_stride, band=8):
    """fcd_duplex_envelope_dev on the viterbi labellings of a pair batch: labels / path rows `stride` apart, envelope rows
    env_stride apart; compact against tests/envelope_model.py, far == compact"""
    import envelope_model as em
    n = nat()
    d = _duplex_data(False, "f16")
    B, T1, T2 = d["B"], d["T1"], d["T2"]
    vit = [[oracle.viterbi_search_raw(np.ascontiguousarray(up[i, :ln[i]]))[:2] for i in range(B)]
           for up, ln in ((d["up1"], d["l1"]), (d["up2"], d["l2"]))]
    got = []
    for W, EW in ((None, None), (stride, env_stride)):
        far = W is not None
        Ws = (T1 if W is None else W, T2 if W is None else W)
        ew = T1 if EW is None else EW
        whole = env.region(max(Ws) * 4 + 5 * SLOT) if far else None
        arrs, lens = [], []
        for side in range(2):
            Tx = (T1, T2)[side]
            lab = _Sub(whole, 2 * side * SLOT) if far else env.region(B * Tx)
            pth = _Sub(whole, (2 * side + 1) * SLOT) if far else env.region(B * Tx * 4)
            for i, (labels, path) in enumerate(vit[side]):
                lab.put(i * Ws[side], np.asarray(labels, np.uint8))
                pth.put(i * Ws[side] * 4, np.asarray(path, np.uint32))
            arrs += [lab, pth]
            lens.append(env.small(np.array([len(v[0]) for v in vit[side]], np.uint32)))
        t1, t2 = env.small(d["l1"]), env.small(d["l2"])
        out = env.region(((B - 1) * ew + T1) * 16)
        rc = env.lib.fcd_duplex_envelope_dev(env.h.ptr, B, C.c_void_p(arrs[0].ptr), C.c_void_p(arrs[1].ptr), C.c_void_p(lens[0].ptr), Ws[0],
                                             C.c_void_p(t1.ptr), T1, C.c_void_p(arrs[2].ptr), C.c_void_p(arrs[3].ptr), C.c_void_p(lens[1].ptr),
                                             Ws[1], C.c_void_p(t2.ptr), T2, band, C.c_void_p(out.ptr), ew)
        assert rc == n.OK, (rc, env.lib.fcd_last_error(env.h.ptr))
        env.sync()
        got.append([out.get(i * ew * 16, np.uint64, 2 * int(d["l1"][i])).reshape(-1, 2) for i in range(B)])
        env.reset()
    for i in range(B):
        want = em.envelope(vit[0][i][0], vit[0][i][1], int(d["l1"][i]), vit[1][i][0], vit[1][i][1], int(d["l2"][i]), band)
        assert np.array_equal(got[0][i], np.asarray(want, np.uint64)), ("envelope", i)
        assert np.array_equal(got[1][i], got[0][i]), ("envelope, far", i, stride, env_stride)


# ---- what the table holds, entry point by entry point ------------------------------------------------------------------
# tests/test_far_offsets_emu.py reads include/fcd.h: every fcd_*_dev declared there is a key of COVERED (the quantities its
# cases take far) or of EXEMPT (why it has none)
_SEARCH = ("in.stride_read", "in.stride_t", "out.out_stride")
_LATTICE = ("in.stride_read", "in.stride_t", "y.stride")
COVERED = {
    "fcd_viterbi_search_dev": _SEARCH,
    "fcd_beam_search_dev": _SEARCH + ("the tree arena",),
    "fcd_crf_beam_search_dev": _SEARCH,
    "fcd_beam_search_nbest_dev": _SEARCH,
    "fcd_crf_beam_search_nbest_dev": _SEARCH,
    "fcd_crf_greedy_search_dev": _SEARCH,
    "fcd_crf_viterbi_search_dev": _SEARCH,
    "fcd_beam_session_push_dev": ("chunk.stride_read",),
    "fcd_beam_session_result_dev": ("the result of chunks pushed from a far buffer",),
    "fcd_ctc_score_dev": _LATTICE,
    "fcd_ctc_align_dev": _LATTICE,
    "fcd_ctc_posterior_dev": _LATTICE,
    "fcd_ctc_edits_dev": _LATTICE,
    "fcd_ctc_occupancy_dev": ("in.stride_read", "in.stride_t", "out.stride_row", "out.stride_t"),
    "fcd_crf_score_dev": _LATTICE,
    "fcd_crf_align_dev": _LATTICE,
    "fcd_crf_posterior_dev": _LATTICE,
    "fcd_crf_edits_dev": _LATTICE,
    "fcd_crf_occupancy_dev": ("in.stride_read", "in.stride_t", "out.stride_row", "out.stride_t"),
    "fcd_crf_transition_probs_dev": ("scores.stride_read", "scores.stride_t", "out.stride_read", "out.stride_t", "out.init_stride"),
    "fcd_crf_marginals_dev": ("scores.stride_read", "scores.stride_t", "out.stride_read", "out.stride_t", "out.emit_stride"),
    "fcd_beam_search_duplex_dev": ("in1 / in2 stride_read", "in1 / in2 stride_t"),
    "fcd_crf_beam_search_duplex_dev": ("in1 / in2 stride_read", "in1 / in2 stride_t"),
    "fcd_duplex_envelope_dev": ("stride1 / stride2", "env_stride"),
    "fcd_result_offsets_dev": ("out_stride",),
    "fcd_pack_results_dev": ("res.out_stride",),
    "fcd_unpack_results_dev": ("out.out_stride",),
}
EXEMPT = {
    "fcd_crf_beam_search_dev_k": "fcd_crf_beam_search_dev is this call with FCD_KERNEL_AUTO: one body, in the table under that name",
    "fcd_gather_results_dev": "needs a communicator and a second rank; its offsets and pack steps are the kernels of fcd_result_offsets_dev / fcd_pack_results_dev",
    "fcd_unpack_gathered_dev": "the unpack step of a gather over several ranks' shards, driven by the distributed tests; no far case yet",
}
