"""TEST INFRASTRUCTURE shared by tests/test_crf_marginals_emu.py (the kernel on the wave64 emulator),
tests/test_gpu_crf_marginals.py (on the GPU) and tests/test_crf_marginals_reference.py (the float32 restatement on the same
table): seeded cases run through fcd_crf_marginals_host / _dev and crf_marginals_batch_raw and compared with the float64
restatement tests/crf_marginals_reference.py.  The inputs, their strides and the three reads of lengths (T, T - 3, 0) per
case are tests/crf_transitions_cases.py's.

The table: rows of at most 64 elements (a lane per element: (4, 5), (3, 2) with nb = 1, (12, 5) with 60), one chunk of states
((16, 5) with idle lanes, (64, 5) exactly), a partial last chunk ((80, 9); (8, 9), 72 elements on 8 lanes), many chunks
((256, 5), (1024, 3), (4096, 5)) and the launch whose LDS passes 64 KiB ((8704, 3)); lengths from {1, 2, 3, 7, 65, 130, 300}.

Allowance on marg and emit (absolute): 4 err32 + 2^-20, err32 the case's largest difference between the float32 restatement
and the float64 reference -- the backward half's exp, ln and division are within about 2 ulp on the device where libm is
within 0.5 and enter as the restatement's roundings do, the forward half is products and sums that the restatement rounds
exactly as the device does.  logZ: 2^-20 max(1, |logZ|)."""
import ctypes as C

import numpy as np

import crf_marginals_reference as M
import crf_transitions_cases as TC
import crf_transitions_reference as R

SENTINEL = TC.SENTINEL  # what the output rows hold before the call: no probability


def _case(name, S, N, T, **kw):
    return TC._case("m_" + name, S, N, T, **kw)


CASES = [
    # a lane per element
    _case("s4_n5_t1", 4, 5, 1),
    _case("s4_n5_t7_dest_f16", 4, 5, 7, sd=5.0, dtype="f16", layout="dest"),
    _case("s4_n5_t300_tm", 4, 5, 300, tm_in=True, tm_out=True),
    _case("s3_n2_t1_dest", 3, 2, 1, layout="dest"),
    _case("s3_n2_t300_bf16", 3, 2, 300, sd=5.0, dtype="bf16"),
    _case("s12_n5_t7_dest_padded", 12, 5, 7, layout="dest", padded=True),
    # a lane per state, one chunk
    _case("s16_n5_t2_tm", 16, 5, 2, tm_in=True, tm_out=True),
    _case("s16_n5_t65_dest_sd5", 16, 5, 65, sd=5.0, layout="dest"),
    _case("s16_n5_t300_f16", 16, 5, 300, dtype="f16"),
    _case("s64_n5_t2_bf16_padded", 64, 5, 2, dtype="bf16", padded=True),
    _case("s64_n5_t65", 64, 5, 65),
    _case("s64_n5_t300_sd5", 64, 5, 300, sd=5.0),
    _case("s64_n5_t65_forbidden_dest", 64, 5, 65, forbidden=True, layout="dest"),
    _case("s16_n5_t65_shift1000", 16, 5, 65, shift=1000.0),
    # a partial last chunk
    _case("s80_n9_t7_dest", 80, 9, 7, layout="dest"),
    _case("s8_n9_t65_bf16", 8, 9, 65, dtype="bf16"),
    # many chunks
    _case("s256_n5_t65_dest_tm", 256, 5, 65, sd=5.0, layout="dest", tm_in=True, tm_out=True),
    _case("s1024_n3_t130_f16_dest", 1024, 3, 130, dtype="f16", layout="dest"),
    _case("s4096_n5_t3_f16", 4096, 5, 3, dtype="f16"),
]
# 8 S + 4608 bytes of LDS per read: S = 8704 is the smallest multiple of 512 that takes the launch past 64 KiB
BIG_LDS = _case("s8704_n3_t2_f16_big_lds", 8704, 3, 2, dtype="f16")


def by_name(name):
    return [k for k in CASES if k["name"] == "m_" + name][0]


logz_bound = TC.logz_bound
_built = {}


def build_case(case):
    """-> the case with its inputs and references (computed once and shared: do not modify)"""
    if case["name"] in _built:
        return _built[case["name"]]
    c = dict(TC.build_case(case))
    x, lengths = c["x32"], c["lengths"]
    c["mrefs"] = [M.marginals64(x[b, :lengths[b]]) for b in range(c["B"])]
    c["mrefs32"] = [M.marginals32(x[b, :lengths[b]], c["refs32"][b]) for b in range(c["B"])]
    err = 0.0
    for ref, r32 in zip(c["mrefs"], c["mrefs32"]):
        if ref["ok"] and r32["ok"] and ref["marg"].size:
            err = max(err, float(np.abs(r32["marg"] - ref["marg"]).max()), float(np.abs(r32["emit"] - ref["emit"]).max()))
    c["merr32"] = err
    _built[case["name"]] = c
    return c


OBSERVED = {}  # case name -> the largest error on marg and emit the last run_case saw (the figures of INTEGRATION.md 2l)


def check_read(c, b, marg, emit, logz, status, where):
    """one read of a result (numpy arrays; marg (T, S, N), emit (T, N) or None) against the float64 reference"""
    ref = c["mrefs"][b]
    Tr, S, N = int(c["lengths"][b]), c["S"], c["N"]
    assert ref["ok"] and int(status) == 0, where
    tol = 4 * c["merr32"] + 2.0 ** -20
    assert marg.dtype == np.float32
    assert (marg[Tr:] == SENTINEL).all(), (where, "rows of marg at and beyond T_r were written")
    if logz is not None:
        assert abs(logz - ref["logz"]) <= logz_bound(ref["logz"]), (where, "logz", logz, ref["logz"])
    worst = 0.0
    if Tr:
        m = marg[:Tr].astype(np.float64)
        assert ((m >= 0) & (m <= 1)).all(), where
        worst = float(np.abs(m - ref["marg"]).max())
        assert worst <= tol, (where, "marg", worst, tol)
        rows = np.abs(m.sum(axis=(1, 2)) - 1.0).max()
        assert rows <= tol * S * N, (where, "a row of marg does not sum to 1", rows)
        assert (marg[:Tr][np.isneginf(c["x32"][b, :Tr])] == 0).all(), (where, "a forbidden transition has a marginal")
    if emit is not None:
        assert emit.dtype == np.float32
        assert (emit[Tr:] == SENTINEL).all(), (where, "rows of emit at and beyond T_r were written")
        if Tr:
            e = emit[:Tr].astype(np.float64)
            we = float(np.abs(e - ref["emit"]).max())
            assert we <= tol, (where, "emit", we, tol)
            worst = max(worst, we)
            own = float(np.abs(e - marg[:Tr].astype(np.float64).sum(axis=1)).max())
            assert own <= S * 2.0 ** -23, (where, "emit is not the sum of the returned marg over states", own)
    OBSERVED[c["name"]] = max(OBSERVED.get(c["name"], 0.0), worst)


def call_abi(fcd, c, device=None, want_logz=True, want_emit=True, pad_out=False):
    """The C ABI on the case: sentinel-filled marg with the case's output strides (tm_out: (T, B, S, N); pad_out: spare
    elements between rows and reads, of emit too) -> marg (B, T, S, N) view, emit (B, T, N) view, logz, status as numpy arrays
    (emit and logz sentinel-filled where not asked for)"""
    from fast_ctc_decode_amd import _native as nat
    B, T, S, N = c["B"], c["T"], c["S"], c["N"]
    xin = c["xin"]
    if c["tm_out"]:
        buf = np.full((T, B, S * N + (3 if pad_out else 0)), SENTINEL, np.float32)
        stride_t, stride_read = buf.strides[0] // 4, buf.strides[1] // 4
        view = lambda a: a[:, :, :S * N].reshape(T, B, S, N).transpose(1, 0, 2, 3)
    else:
        buf = np.full((B, T + (1 if pad_out else 0), S * N + (3 if pad_out else 0)), SENTINEL, np.float32)
        stride_read, stride_t = buf.strides[0] // 4, buf.strides[1] // 4
        view = lambda a: a[:, :T, :S * N].reshape(B, T, S, N)
    stride_read, stride_t = max(stride_read, S * N), max(stride_t, S * N)
    em = np.full((B, T * N + (5 if pad_out else 0)), SENTINEL, np.float32)
    logz = np.full(B, SENTINEL, np.float64)
    status = np.full(B, -1, np.int32)
    st = [s // xin.itemsize for s in xin.strides]
    dcode = {"f32": nat.DTYPE_F32, "f16": nat.DTYPE_F16, "bf16": nat.DTYPE_BF16}[c["dtype"]]
    layout = nat.LAYOUT_DEST if c["layout"] == "dest" else nat.LAYOUT_SOURCE
    if device is None:
        h = nat.default_handle()
        fn = h.lib.fcd_crf_marginals_host
        keep = (xin, c["lengths"], buf, em, logz, status)
        ptr = lambda a: a.ctypes.data
    else:
        import torch
        h = nat.default_handle(0)
        fn = h.lib.fcd_crf_marginals_dev
        xd = TC._device_array(xin if c["dtype"] != "bf16" else xin.view(np.int16), device)
        keep = (xd,) + tuple(torch.from_numpy(a).to(device) for a in (c["lengths"], buf, em, logz, status))
        ptr = lambda a: a.data_ptr()
        h.set_stream(torch.cuda.current_stream().cuda_stream)
    b = nat.Batch(ptr(keep[0]), B, T, S, N, st[0], st[1], st[2], st[3], ptr(keep[1]), dcode)
    out = nat.Marginals(ptr(keep[2]), stride_read, stride_t, ptr(keep[3]) if want_emit else None, em.shape[1],
                        ptr(keep[4]) if want_logz else None, ptr(keep[5]))
    rc = fn(h.ptr, C.byref(b), layout, C.byref(out))
    assert rc == nat.OK, (rc, h.lib.fcd_last_error(h.ptr))
    if device is not None:
        torch.cuda.synchronize()
        buf, em, logz, status = (a.cpu().numpy() for a in keep[2:])
    assert (em[:, T * N:] == SENTINEL).all(), "the spare elements between the reads of emit were written"
    if pad_out:  # nothing outside the strided rows
        assert (buf[..., S * N:] == SENTINEL).all(), "the spare elements between the rows of marg were written"
        assert c["tm_out"] or (buf[:, T:] == SENTINEL).all(), "the spare row between the reads of marg was written"
    return view(buf), em[:, :T * N].reshape(B, T, N), logz, status


def call_api(fcd, c, device=None, emit=True):
    """crf_marginals_batch_raw on the case -> a MarginalResult of numpy arrays"""
    kw = dict(layout=c["layout"], time_major_out=c["tm_out"], emit=emit)
    if device is None:
        if c["dtype"] == "bf16":
            kw["input_dtype"] = "bfloat16"
        return fcd.crf_marginals_batch_raw(c["xin"], c["lengths"], **kw)
    import torch
    xd = TC._device_array(c["xin"] if c["dtype"] != "bf16" else c["xin"].view(np.int16), device)
    if c["dtype"] == "bf16":
        xd = xd.view(torch.bfloat16)
    r = fcd.crf_marginals_batch_raw(xd, torch.from_numpy(c["lengths"]).to(device), **kw)
    assert r.marginals.is_cuda and r.logz.is_cuda and r.status.is_cuda and (r.emit is None or r.emit.is_cuda)
    return r.cpu()


def call_transitions(fcd, c, device=None):
    """crf_transition_probs_batch_raw (float32 probabilities) on the case -> a TransitionResult of numpy arrays"""
    assert c["out"] == "f32"
    return TC.call_api(fcd, c, device)


def run_case(fcd, case, device=None):
    """The C ABI (sentinel rows, the case's strides) against the reference; the Python function against the C ABI: the same
    bits wherever the call writes; crf_transition_probs on the same scores: logz and status bit for bit, and its (probs,
    init) propagated forward in numpy are the same marg bit for bit.  -> (marg, emit, logz, status) of the C ABI call"""
    c = build_case(case)
    marg, emit, logz, status = call_abi(fcd, c, device)
    for b in range(c["B"]):
        check_read(c, b, marg[b], emit[b], float(logz[b]), status[b], (c["name"], b))
    assert int(c["lengths"][2]) == 0 and logz[2] == np.log(float(c["S"]))
    r = call_api(fcd, c, device)
    assert r.marginals.shape == marg.shape and r.marginals.dtype == marg.dtype and r.emit.shape == emit.shape
    tr = call_transitions(fcd, c, device)
    for b in range(c["B"]):
        n = int(c["lengths"][b])
        assert np.array_equal(r.marginals[b, :n], marg[b, :n]), (c["name"], b, "the Python function and the C ABI differ")
        assert np.array_equal(r.emit[b, :n], emit[b, :n]), (c["name"], b)
        want, _ = M.propagate32(tr.probs[b, :n], tr.init[b])
        assert np.array_equal(want, marg[b, :n]), (c["name"], b, "not the forward propagation of crf_transition_probs' output")
    assert np.array_equal(r.logz, logz) and np.array_equal(r.status, status)
    assert np.array_equal(tr.logz, logz) and np.array_equal(tr.status, status)
    return marg, emit, logz, status


def edge_cases(fcd, device=None):
    """a NaN row, a +inf, a row nothing passes, T_r = 0, failed reads beside good ones, -inf scores, the single-read function"""
    to = TC._conv(device)
    rng = np.random.default_rng(19)
    for S, N, T in ((4, 5, 9), (64, 5, 6), (256, 3, 5)):
        good = R.random_scores(rng, T, S, N)
        x = np.stack([good] * 6)
        x[1, 2] = np.nan                    # a NaN row
        x[2, T - 1, S - 1, N - 1] = np.inf  # one +inf
        x[3, 1] = -np.inf                   # a row nothing passes: no path has positive weight
        x[4, 0, 0, 0] = np.nan              # ... beyond the read's length: not looked at
        lengths = np.array([T, T, T, T, 0, T], np.int64)
        r = fcd.crf_marginals_batch_raw(to(x), to(lengths)).cpu()
        solo = fcd.crf_marginals_batch_raw(to(good[None])).cpu()
        assert r.status.tolist() == [0, 2, 2, 2, 0, 0], (S, r.status)
        assert np.isnan(r.logz[1:4]).all() and r.logz[4] == np.log(float(S))
        for b in (0, 5):  # the good reads are what they are on their own
            assert np.array_equal(r.marginals[b], solo.marginals[0]) and np.array_equal(r.emit[b], solo.emit[0])
            assert r.logz[b] == solo.logz[0]
        ref = M.marginals64(good)
        assert np.abs(r.marginals[0] - ref["marg"]).max() < 1e-5 and np.abs(r.emit[0] - ref["emit"]).max() < 1e-5
        assert abs(r.logz[0] - ref["logz"]) <= logz_bound(ref["logz"])
        # a -inf score alone fails nothing: its marginal is exactly 0, and so is every edge out of a dead state
        y = good.copy()
        y[T - 2, 1, :] = -np.inf
        y[0, 2, 1] = -np.inf
        y[0, 3, :] = -np.inf  # dead at row 0
        d = fcd.crf_marginals_batch_raw(to(y[None])).cpu()
        assert int(d.status[0]) == 0 and (d.marginals[0, T - 2, 1] == 0).all() and d.marginals[0, 0, 2, 1] == 0
        assert (d.marginals[0, 0, 3] == 0).all()
        ref = M.marginals64(y)
        assert np.abs(d.marginals[0] - ref["marg"]).max() < 1e-5 and abs(d.logz[0] - ref["logz"]) <= logz_bound(ref["logz"])
        assert np.abs(d.marginals[0].astype(np.float64).sum(axis=(1, 2)) - 1.0).max() < 1e-5
    import pytest
    if device is None:
        marg, emit, logz = fcd.crf_marginals(good)
        assert marg.shape == good.shape and emit.shape == (good.shape[0], good.shape[2]) and isinstance(logz, float)
        assert np.array_equal(marg, solo.marginals[0]) and np.array_equal(emit, solo.emit[0]) and logz == solo.logz[0]
        md, ed, lzd = fcd.crf_marginals(R.source_to_dest(good), layout="dest")
        assert np.array_equal(md, marg) and np.array_equal(ed, emit) and lzd == logz
        with pytest.raises(RuntimeError, match="Failed to compare values"):
            fcd.crf_marginals(x[1])


def nullable_outputs(fcd, device=None):
    """out->emit and out->logz are nullable: the other outputs are the same bits with and without them; spare elements
    between rows and reads stay untouched (call_abi checks them)"""
    for name in ("s16_n5_t65_dest_sd5", "s4_n5_t300_tm", "s256_n5_t65_dest_tm"):
        c = build_case(by_name(name))
        full = call_abi(fcd, c, device)
        for want_logz, want_emit, pad_out in ((False, True, False), (True, False, True), (False, False, False), (True, True, True)):
            got = call_abi(fcd, c, device, want_logz=want_logz, want_emit=want_emit, pad_out=pad_out)
            for b in range(c["B"]):
                n = int(c["lengths"][b])
                assert np.array_equal(got[0][b, :n], full[0][b, :n]) and (got[0][b, n:] == SENTINEL).all()
                assert np.array_equal(got[1][b, :n], full[1][b, :n]) if want_emit else (got[1] == SENTINEL).all()
            assert np.array_equal(got[3], full[3])
            assert np.array_equal(got[2], full[2]) if want_logz else (got[2] == SENTINEL).all()
        r = call_api(fcd, c, device, emit=False)
        assert r.emit is None and np.array_equal(r.logz, full[2])


def argument_errors(fcd, device=None):
    """the argument errors at both layers, and every limit"""
    import pytest
    from fast_ctc_decode_amd import _native as nat
    to = TC._conv(device)
    x = R.random_scores(np.random.default_rng(3), 6, 4, 5)
    xb = to(x[None])
    with pytest.raises(ValueError, match="layout"):
        fcd.crf_marginals_batch_raw(xb, layout="both")
    with pytest.raises(ValueError, match="lengths must have shape"):
        fcd.crf_marginals_batch_raw(xb, to(np.array([1, 2], np.int64)))
    with pytest.raises(TypeError):
        fcd.crf_marginals_batch_raw(to(x))  # rank 3
    if device is None:
        with pytest.raises(TypeError):
            fcd.crf_marginals_batch_raw(x.astype(np.float64)[None])
        with pytest.raises(TypeError):
            fcd.crf_marginals(x[None])  # rank 4
        with pytest.raises(TypeError):
            fcd.crf_logz(x[None])  # not a device tensor

    def wide(shape):  # one element seen as a large array: the limits are refused before anything is read
        if device is None:
            return np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape, (0, 0, 0, 0))
        import torch
        return torch.zeros(1, device=device).expand(shape)
    for shape, words in (((1, 2, 5, 4), "multiple of N - 1"), ((1, 2, 9, 10), "2 .. 9"), ((1, 2, 4, 1), "2 .. 9"),
                         ((1, 1, 1 << 24, 2), "below 2^24"), ((1, 1, 20480, 3), "LDS")):
        with pytest.raises(nat.NativeError) as e:
            fcd.crf_marginals_batch_raw(wide(shape))
        assert e.value.code == nat.E_UNSUPPORTED and "crf_marginals" in str(e.value) and words in str(e.value), shape
    r = fcd.crf_marginals_batch_raw(wide((1, 1, 19904, 3))).cpu()  # the largest S the LDS holds
    assert int(r.status[0]) == 0 and abs(float(r.marginals[0, 0].sum()) - 1.0) < 1e-4 and abs(r.logz[0] - np.log(3 * 19904.0)) < 1e-5
    assert np.abs(r.emit[0, 0] - 1.0 / 3).max() < 1e-5
    # the C ABI itself
    h = nat.default_handle() if device is None else nat.default_handle(0)
    fn = h.lib.fcd_crf_marginals_host if device is None else h.lib.fcd_crf_marginals_dev
    arrays = (x, np.zeros((6, 4, 5), np.float32), np.zeros((6, 5), np.float32), np.zeros(1), np.zeros(1, np.int32))
    if device is None:
        keep = list(arrays)
        ptr = lambda a: a.ctypes.data
    else:
        import torch
        keep = [torch.from_numpy(a).to(device) for a in arrays]
        ptr = lambda a: a.data_ptr()
    xp, mp, ep, zp, sp = (ptr(a) for a in keep)
    b = nat.Batch(xp, 1, 6, 4, 5, 120, 20, 5, 1, None)

    def mg(marg=mp, stride_read=120, stride_t=20, emit=ep, emit_stride=30, logz=zp, status=sp):
        return nat.Marginals(marg, stride_read, stride_t, emit, emit_stride, logz, status)
    assert fn(h.ptr, C.byref(b), 0, C.byref(mg())) == nat.OK
    assert fn(h.ptr, C.byref(b), 0, C.byref(mg(emit=None, emit_stride=0, logz=None))) == nat.OK
    assert fn(h.ptr, None, 0, C.byref(mg())) == nat.E_INVALID
    assert fn(h.ptr, C.byref(b), 0, None) == nat.E_INVALID
    for bad in (mg(marg=None), mg(status=None), mg(stride_read=19), mg(stride_t=19), mg(emit_stride=29)):
        assert fn(h.ptr, C.byref(b), 0, C.byref(bad)) == nat.E_INVALID
    for layout in (-1, 2):
        assert fn(h.ptr, C.byref(b), layout, C.byref(mg())) == nat.E_INVALID
    assert fn(h.ptr, C.byref(nat.Batch(None, 1, 6, 4, 5, 120, 20, 5, 1, None)), 0, C.byref(mg())) == nat.E_INVALID  # null scores
    bad_dtype = nat.Batch(xp, 1, 6, 4, 5, 120, 20, 5, 1, None, 9)
    assert fn(h.ptr, C.byref(bad_dtype), 0, C.byref(mg())) == nat.E_INVALID
    assert fn(h.ptr, C.byref(nat.Batch(xp, 1, 6, 4, 5, 120, -20, 5, 1, None)), 0, C.byref(mg())) == nat.E_INVALID
    empty = nat.Batch(None, 0, 6, 4, 5, 120, 20, 5, 1, None)
    assert fn(h.ptr, C.byref(empty), 0, C.byref(mg(marg=None, status=None))) == nat.OK  # no reads: nothing to do
