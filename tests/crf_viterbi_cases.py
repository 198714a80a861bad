"""TEST INFRASTRUCTURE shared by tests/test_crf_viterbi_emu.py (the kernel on the wave64 emulator) and
tests/test_gpu_crf_viterbi.py (on the GPU): seeded cases run through crf_viterbi_search_batch_raw and compared with the
restatement tests/crf_viterbi_reference.py.

status, out_len, labels, path and qual must equal the restatement EXACTLY (the kernel's arithmetic is the restatement's: f32
mantissa products, exact rescaling, the same tie rules); logp within 2^-40 relative, the figure recorded for the project's
float64 log forms (the kernel and libm may round the logarithm's last bit differently).  Posteriors are Dirichlet(0.5) rows
floored at 2^-20; asserted for every read: the restatement with drop=2^-160 returns the same result -- no case relies on
cells the contract lets the kernel drop.
Cross-checks on the results: crf_align of the returned labelling (band 0) returns the path as start and the same qual
exactly, and the same logp within 2^-40 relative; its crf_score is at least that logp (within the score's own bound of
4 T_r 2^-24 nats, crf_lattice_cases.tolerance); crf_greedy_search on the same inputs still returns what
search::crf_greedy_search's restatement does.

A case: (name, S, N, T, dtype, layout); B = 3 reads of lengths (T, T - 3, 0)."""
import ctypes as C
import math

import numpy as np

import crf_lattice_cases as CC
import crf_viterbi_reference as R

DTYPES = ("f32", "f16", "bf16")


def _grid():
    out = []
    for i_s, S in enumerate((4, 16, 64, 256, 1024)):
        for i_n, N in enumerate((2, 3, 5)):
            for i_t, T in enumerate((1, 2, 63, 64, 65, 300)):
                # (the element types and the two storage orders go round the grid: every S, N and T meets each of them)
                dtype = DTYPES[(i_s + i_n + i_t) % 3]
                layout = "time" if (i_s + 2 * i_n + i_t) % 2 else "read"
                out.append(("s%dn%d_t%d_%s_%s" % (S, N, T, dtype, layout), S, N, T, dtype, layout))
    for i_t, T in enumerate((1, 2, 63, 64, 65, 300)):
        out.append(("s64n9_t%d_%s" % (T, DTYPES[i_t % 3]), 64, 9, T, DTYPES[i_t % 3], "time" if i_t % 2 else "read"))
        out.append(("s12n5_t%d_%s" % (T, DTYPES[(i_t + 1) % 3]), 12, 5, T, DTYPES[(i_t + 1) % 3], "read" if i_t % 2 else "time"))
    return out


CASES = _grid()
BIG_LDS = ("s4096n5_t64_f16_read", 4096, 5, 64, "f16", "read")  # N S 4 = 80 KiB: the launch that raises the kernel's LDS limit

_built = {}


def build_case(case):
    """-> dict with the inputs and the restatement's results; built once per process, shared, never changed"""
    name, S, N, T, dtype, layout = case
    if name in _built:
        return _built[name]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    B = 3
    x = np.stack([R.random_case(rng, T, S, N)[0] for _ in range(B)])
    if dtype == "f16":
        xin = x.astype(np.float16)
        x32 = xin.astype(np.float32)
    elif dtype == "bf16":
        bits = (x.view(np.uint32) >> 16).astype(np.uint16)  # truncation: any bf16 value will do
        xin, x32 = bits, (bits.astype(np.uint32) << 16).view(np.float32)
    else:
        xin = x32 = x
    assert (x32 >= 2.0 ** -20).all()
    if layout == "time":
        xin = np.ascontiguousarray(xin.transpose(1, 0, 2, 3)).transpose(1, 0, 2, 3)
    init = rng.random((B, S)).astype(np.float32)
    lengths = np.array([T, max(T - 3, 0), 0], np.int64)
    refs = []
    for b in range(B):
        ref = R.viterbi(x32[b, :lengths[b]], init[b])
        cond = R.viterbi(x32[b, :lengths[b]], init[b], drop=2.0 ** -160)
        assert ref["labels"] == cond["labels"] and ref["path"] == cond["path"], ("the case relies on dropped cells", name, b)
        refs.append(ref)
    c = dict(name=name, S=S, N=N, T=T, B=B, dtype=dtype, xin=xin, x32=x32, init=init, lengths=lengths, refs=refs)
    _built[name] = c
    return c


def same_logp(got, want):
    if want != want or math.isinf(want) or want == 0.0:
        return (got != got) if want != want else got == want
    return abs(got - want) <= 2.0 ** -40 * abs(want)


def check_read(r, b, ref, where):
    """read b of a result on numpy arrays against the restatement's dict"""
    n = int(r.out_len[b])
    assert int(r.status[b]) == ref["status"], where
    assert n == len(ref["labels"]), where
    assert r.labels[b, :n].tolist() == ref["labels"], where
    assert np.asarray(r.path[b, :n]).astype(np.int64).tolist() == ref["path"], where
    assert np.asarray(r.qual[b, :n]).view(np.uint32).tolist() == np.asarray(ref["qual"], np.float32).view(np.uint32).tolist(), where
    assert same_logp(float(r.logp[b]), ref["logp"]), where + (float(r.logp[b]), ref["logp"])


def run_case(fcd, c, device=None, cross=True):
    xin, conv, kw = CC._device_inputs(c, device)
    init, lengths = conv(c["init"]), conv(c["lengths"])
    r = fcd.crf_viterbi_search_batch_raw(xin, init, lengths, qual=True, **kw)
    if device is not None:
        import torch
        assert r.labels.device == xin.device and r.logp.dtype == torch.float64 and r.logp.shape == (c["B"],)
    rc = r.cpu()
    assert rc.logp.dtype == np.float64 and rc.logp.shape == (c["B"],) and rc.qual.dtype == np.float32
    for b in range(c["B"]):
        check_read(rc, b, c["refs"][b], (c["name"], b))
    if not cross:
        return rc
    # the labelling's own best alignment is the path, and all of its alignments together weigh no less
    al = r.crf_align(xin, init, lengths=lengths, **kw).cpu()
    sc = r.crf_score(xin, init, lengths=lengths, **kw)
    sc = sc if isinstance(sc, np.ndarray) else sc.cpu().numpy()
    for b in range(c["B"]):
        n, Tr = int(rc.out_len[b]), int(c["lengths"][b])
        where = (c["name"], b, "crf_align")
        assert al.start[b, 0, :n].tolist() == np.asarray(rc.path[b, :n]).astype(np.uint32).tolist(), where
        assert al.qual[b, 0, :n].view(np.uint32).tolist() == np.asarray(rc.qual[b, :n]).view(np.uint32).tolist(), where
        assert same_logp(float(al.logp[b, 0]), float(rc.logp[b])), where + (al.logp[b, 0], rc.logp[b])
        assert sc[b, 0] >= rc.logp[b] - CC.tolerance(Tr), (c["name"], b, "crf_score", sc[b, 0], rc.logp[b])
    # crf_greedy_search on the same inputs: what it always returned
    if c["dtype"] != "bf16":
        g = fcd.crf_greedy_search_batch_raw(xin, init, lengths, qual=True).cpu()
        for b in range(c["B"]):
            labels, path, qual, logw = R.greedy(c["x32"][b, :c["lengths"][b]], c["init"][b])
            n = int(g.out_len[b])
            where = (c["name"], b, "greedy")
            assert int(g.status[b]) == 0 and g.labels[b, :n].tolist() == labels, where
            assert np.asarray(g.path[b, :n]).astype(np.int64).tolist() == path, where
            assert np.asarray(g.qual[b, :n]).view(np.uint32).tolist() == np.asarray(qual, np.float32).view(np.uint32).tolist(), where
            assert rc.logp[b] >= logw - CC.tolerance(int(c["lengths"][b])), where  # greedy's path is one of the paths
    return rc


def _conv(device):
    if device is None:
        return lambda a: a
    import torch
    return lambda a: None if a is None else torch.from_numpy(a).to(device)


def edge_cases(fcd, device=None):
    """every edge case of the definition, one read each, in one batch"""
    rng = np.random.default_rng(77)
    to = _conv(device)
    S, N, T, B = 16, 5, 12, 9
    x = np.stack([R.random_case(rng, T, S, N)[0] for _ in range(B)])
    init = rng.random((B, S + 2)).astype(np.float32)
    init[:, S:] = 0.0
    lengths = np.full(B, T, np.int64)
    init[1, 3] = np.nan                      # 1: NaN in the init row
    init[2, S + 1] = 5.0                     # 2: the first maximum lies beyond the states
    lengths[3] = 0                           # 3: no rows ...
    init[4, S + 1], lengths[4] = 5.0, 0      # 4: ... and then the init row's state is never read
    x[5, 7, 9, 2] = np.nan                   # 5: a NaN inside the read
    x[6, 10, 3, 1], lengths[6] = np.nan, 10  # 6: a NaN beyond the read's rows: not read
    x[7, 4, :, 3] = np.inf                   # 7: infinite posteriors
    x[8, 5, :, 0] = -0.25                    # 8: negative posteriors
    r = fcd.crf_viterbi_search_batch_raw(to(x), to(init), to(lengths), qual=True).cpu()
    for b in (0, 1, 2, 3, 4, 5, 6):
        check_read(r, b, R.viterbi(x[b, :lengths[b]], init[b]), ("edge", b))
    assert [int(s) for s in r.status[:7]] == [0, R.ST_BAD_STATE, R.ST_BAD_STATE, 0, 0, R.ST_INCOMPARABLE, 0]
    assert math.isnan(r.logp[1]) and math.isnan(r.logp[2]) and r.logp[3] == 0.0 and r.logp[4] == 0.0 and math.isnan(r.logp[5])
    assert r.out_len[1] == r.out_len[2] == r.out_len[3] == r.out_len[4] == r.out_len[5] == 0
    for b in (7, 8):  # they terminate and write some result, nothing more
        assert int(r.status[b]) in (0, R.ST_INCOMPARABLE) and 0 <= int(r.out_len[b]) <= T
    return r


def tie_rules(fcd, device=None):
    """the tie rules on the kernel itself, on rows whose values are all equal: stay before an equal advance, the lowest i
    among equal advances, the first maximum at the end -- one state per lane, a lane per element, and S > 64, where the end
    state comes out of the reduction across lanes"""
    to = _conv(device)
    for S, N, T, s0 in ((4, 5, 3, 1), (4, 5, 70, 3), (16, 3, 9, 5), (64, 5, 6, 40), (128, 5, 5, 77), (256, 3, 11, 200), (192, 9, 4, 100)):
        x = np.full((2, T, S, N), 0.25, np.float32)
        x[1, :, :, 1:] = 0.125  # read 1: advances lose to stay, so only the end-state rule decides
        init = np.zeros((2, S), np.float32)
        init[:, s0] = 1.0
        r = fcd.crf_viterbi_search_batch_raw(to(x), to(init), qual=True).cpu()
        for b in range(2):
            check_read(r, b, R.viterbi(x[b], init[b]), ("ties", S, N, T, b))
        # read 1: nothing ever beats stay, state s0 keeps all the weight and no label is emitted
        assert int(r.out_len[1]) == 0 and same_logp(float(r.logp[1]), T * math.log(0.25)), (S, N, T)
        # read 0: after m = ceil(log_nb S) rows every state holds the same value; the path ends in the FIRST of them
        assert same_logp(float(r.logp[0]), T * math.log(0.25)), (S, N, T)
    # the smallest case by hand: row 0 carries state 1's weight to every state, the end is state 0, entered at row 0 from
    # state 1 = s_1 with label 1 and kept by stay -- never by an equal advance -- afterwards
    x = np.full((1, 3, 4, 5), 0.25, np.float32)
    r = fcd.crf_viterbi_search_batch_raw(to(x), to(np.array([[0, 1, 0, 0]], np.float32)), qual=True).cpu()
    assert int(r.out_len[0]) == 1 and r.labels[0, :1].tolist() == [1] and np.asarray(r.path[0, :1]).tolist() == [0]


def nullable_outputs(fcd, device=None):
    """every combination of the C ABI's nullable pointers (out->qual, out->path, logp) writes the same values"""
    from fast_ctc_decode_amd import _native as nat
    c = build_case(CASES[0] if device is None else [k for k in CASES if k[1] == 64 and k[2] == 5 and k[3] == 65][0])
    B, T, S, N = c["B"], c["T"], c["S"], c["N"]
    x = np.ascontiguousarray(c["x32"])
    h = nat.default_handle() if device is None else nat.default_handle(0)
    fn = h.lib.fcd_crf_viterbi_search_host if device is None else h.lib.fcd_crf_viterbi_search_dev
    w = max(T, 1)
    if device is not None:
        import torch
        keep = [torch.from_numpy(a).to(device) for a in (x, c["init"], c["lengths"])]
        ptr = lambda a: a.data_ptr()
        h.set_stream(torch.cuda.current_stream().cuda_stream)
    else:
        keep = [x, c["init"], c["lengths"]]
        ptr = lambda a: a.ctypes.data
    for want_qual in (False, True):
        for want_path in (False, True):
            for want_logp in (False, True):
                arrs = dict(labels=np.zeros((B, w), np.uint8), path=np.zeros((B, w), np.int32), qual=np.zeros((B, w), np.float32),
                            out_len=np.zeros(B, np.int32), status=np.full(B, -1, np.int32), logp=np.full(B, 7.0))
                if device is not None:
                    arrs = {k: torch.from_numpy(v).to(device) for k, v in arrs.items()}
                b = nat.Batch(ptr(keep[0]), B, T, S, N, T * S * N, S * N, N, 1, ptr(keep[2]))
                res = nat.Result(ptr(arrs["labels"]), ptr(arrs["path"]) if want_path else None,
                                 ptr(arrs["qual"]) if want_qual else None, ptr(arrs["out_len"]), ptr(arrs["status"]), w, None)
                rc = fn(h.ptr, C.byref(b), C.c_void_p(ptr(keep[1])), S, S, C.byref(res),
                        C.c_void_p(ptr(arrs["logp"])) if want_logp else None)
                assert rc == nat.OK, rc
                if device is not None:
                    torch.cuda.synchronize()
                    arrs = {k: v.cpu().numpy() for k, v in arrs.items()}
                for i in range(B):
                    ref = c["refs"][i]
                    n = int(arrs["out_len"][i])
                    where = ("nullable", want_qual, want_path, want_logp, i)
                    assert int(arrs["status"][i]) == 0 and arrs["labels"][i, :n].tolist() == ref["labels"], where
                    if want_path:
                        assert arrs["path"][i, :n].tolist() == ref["path"], where
                    else:
                        assert (arrs["path"] == 0).all(), where
                    if want_qual:
                        assert arrs["qual"][i, :n].view(np.uint32).tolist() == np.asarray(ref["qual"], np.float32).view(np.uint32).tolist(), where
                    else:
                        assert (arrs["qual"] == 0).all(), where
                    assert same_logp(float(arrs["logp"][i]), ref["logp"]) if want_logp else arrs["logp"][i] == 7.0, where


def argument_errors(fcd, device=None):
    """the argument errors at both layers, and the limits"""
    import pytest
    from fast_ctc_decode_amd import _native as nat
    to = _conv(device)
    rng = np.random.default_rng(3)
    x, init = R.random_case(rng, 6, 4, 5)
    xb, ib = to(x[None]), to(init[None])
    with pytest.raises(ValueError, match="init_states must have shape"):
        fcd.crf_viterbi_search_batch_raw(xb, to(np.ones((2, 4), np.float32)))
    with pytest.raises(nat.NativeError) as e:  # S = 5, N = 4: no multiple of N - 1
        fcd.crf_viterbi_search_batch_raw(to(R.random_case(rng, 6, 5, 4)[0][None]), to(np.ones((1, 5), np.float32)))
    assert e.value.code == nat.E_UNSUPPORTED and "crf_viterbi_search" in str(e.value) and "multiple of N - 1" in str(e.value)
    with pytest.raises(nat.NativeError) as e:  # N = 10
        fcd.crf_viterbi_search_batch_raw(to(R.random_case(rng, 3, 9, 10)[0][None]), to(np.ones((1, 9), np.float32)))
    assert e.value.code == nat.E_UNSUPPORTED and "2 .. 9" in str(e.value)
    with pytest.raises(nat.NativeError) as e:  # N = 1: nothing to emit
        fcd.crf_viterbi_search_batch_raw(to(np.ones((1, 3, 4, 1), np.float32)), to(np.ones((1, 4), np.float32)))
    assert e.value.code == nat.E_UNSUPPORTED
    with pytest.raises(nat.NativeError) as e:  # N S 4 bytes beyond 160 KiB
        fcd.crf_viterbi_search_batch_raw(to(np.ones((1, 1, 8192, 9), np.float32)), to(np.ones((1, 8), np.float32)))
    assert e.value.code == nat.E_UNSUPPORTED and "LDS" in str(e.value)
    with pytest.raises(nat.NativeError) as e:  # an empty init row
        fcd.crf_viterbi_search_batch_raw(xb, to(np.ones((1, 0), np.float32)))
    assert e.value.code == nat.E_INVALID and "init_state missing" in str(e.value)
    if device is None:
        with pytest.raises(TypeError):
            fcd.crf_viterbi_search_batch_raw(x.astype(np.float64)[None], ib)
        with pytest.raises(TypeError):
            fcd.crf_viterbi_search_batch_raw(x, ib)  # rank 3
    # the C ABI itself: null result, null labels, a stride shorter than T
    h = nat.default_handle() if device is None else nat.default_handle(0)
    fn = h.lib.fcd_crf_viterbi_search_host if device is None else h.lib.fcd_crf_viterbi_search_dev
    b = nat.Batch(x.ctypes.data, 1, 6, 4, 5, 120, 20, 5, 1, None)
    lab, olen, stat = np.zeros(6, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.int32)
    good = nat.Result(lab.ctypes.data, None, None, olen.ctypes.data, stat.ctypes.data, 6, None)
    assert fn(h.ptr, C.byref(b), init.ctypes.data, 4, 4, None, None) == nat.E_INVALID
    assert fn(h.ptr, C.byref(b), None, 4, 4, C.byref(good), None) == nat.E_INVALID
    assert fn(h.ptr, C.byref(b), init.ctypes.data, 4, -4, C.byref(good), None) == nat.E_INVALID
    assert fn(h.ptr, None, init.ctypes.data, 4, 4, C.byref(good), None) == nat.E_INVALID
    for res in (nat.Result(None, None, None, olen.ctypes.data, stat.ctypes.data, 6, None),
                nat.Result(lab.ctypes.data, None, None, None, stat.ctypes.data, 6, None),
                nat.Result(lab.ctypes.data, None, None, olen.ctypes.data, None, 6, None),
                nat.Result(lab.ctypes.data, None, None, olen.ctypes.data, stat.ctypes.data, 5, None)):
        assert fn(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(res), None) == nat.E_INVALID
    empty = nat.Batch(None, 0, 6, 4, 5, 120, 20, 5, 1, None)
    assert fn(h.ptr, C.byref(empty), init.ctypes.data, 4, 4, C.byref(good), None) == nat.OK  # no reads: nothing to do


def workspace_groups(fcd, device=None):
    """a workspace cap of one read's back-pointers, then of two: several launches in the same memory, the same values"""
    from fast_ctc_decode_amd import _native as nat
    to = _conv(device)
    rng = np.random.default_rng(9)
    S, N, T, B = 16, 5, 70, 5
    x = np.stack([R.random_case(rng, T, S, N)[0] for _ in range(B)])
    init = rng.random((B, S)).astype(np.float32)
    lengths = np.array([70, 31, 70, 0, 66], np.int64)
    h = nat.default_handle() if device is None else nat.default_handle(0)
    whole = fcd.crf_viterbi_search_batch_raw(to(x), to(init), to(lengths), qual=True).cpu()
    for b in range(B):
        check_read(whole, b, R.viterbi(x[b, :lengths[b]], init[b]), ("whole", b))
    read_bytes = (T * S + 255) // 256 * 256
    for cap in (1, 2 * read_bytes):
        assert h.lib.fcd_debug_set_align_workspace_cap(h.ptr, cap) == nat.OK
        try:
            parts = fcd.crf_viterbi_search_batch_raw(to(x), to(init), to(lengths), qual=True).cpu()
        finally:
            assert h.lib.fcd_debug_set_align_workspace_cap(h.ptr, 0) == nat.OK
        for b in range(B):
            n = int(whole.out_len[b])
            assert int(parts.out_len[b]) == n and int(parts.status[b]) == int(whole.status[b]), (cap, b)
            assert np.array_equal(parts.labels[b, :n], whole.labels[b, :n]) and np.array_equal(parts.path[b, :n], whole.path[b, :n])
            assert np.array_equal(parts.qual[b, :n], whole.qual[b, :n]) and parts.logp[b] == whole.logp[b], (cap, b)
