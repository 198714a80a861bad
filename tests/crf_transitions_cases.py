"""TEST INFRASTRUCTURE shared by tests/test_crf_transitions_emu.py (the kernel on the wave64 emulator),
tests/test_gpu_crf_transitions.py (on the GPU) and tests/test_crf_transitions_reference.py (the float32 restatement on the same
table): seeded cases run through fcd_crf_transition_probs_host / _dev and crf_transition_probs_batch_raw and compared with
the float64 restatement tests/crf_transitions_reference.py.

The table holds the smallest shapes at which the walk takes another path: rows of at most 64 elements (a lane per element:
(4, 5), (3, 2), (12, 5) with 60), just past it ((16, 5), 80 elements, one chunk of states), exactly one chunk ((64, 5)),
several states per lane ((256, 5), (1024, 3)), the widest row ((8, 9)), nb = 1 ((3, 2)); lengths from {1, 2, 7, 65, 130, 300},
a short and a long one per shape, B = 3 reads of lengths (T, T - 3, 0).

Allowance on p and init (absolute): 4 err32 + 2^-20, err32 the case's largest difference between the float32 restatement and
the float64 reference -- the device's exp, ln and division are within about 2 ulp where libm is within 0.5, and enter p as
the restatement's roundings do; a float16 output adds half a float16 ulp of the value.  logZ: 2^-20 max(1, |logZ|)."""
import ctypes as C

import numpy as np

import crf_transitions_reference as R

SENTINEL = 7.5  # what the output rows hold before the call: exact in float32 and float16, and no probability


def _case(name, S, N, T, sd=2.0, dtype="f32", layout="source", out="f32", tm_in=False, tm_out=False, padded=False, shift=0.0,
          forbidden=False, seed=0):
    return dict(name=name, S=S, N=N, T=T, sd=sd, dtype=dtype, layout=layout, out=out, tm_in=tm_in, tm_out=tm_out,
                padded=padded, shift=shift, forbidden=forbidden, seed=seed)


CASES = [
    _case("s4_n5_t1", 4, 5, 1),
    _case("s4_n5_t7_dest_f16in", 4, 5, 7, sd=5.0, dtype="f16", layout="dest"),
    _case("s4_n5_t300_f16out", 4, 5, 300, out="f16"),
    _case("s4_n5_t130_forbidden", 4, 5, 130, forbidden=True),
    _case("s16_n5_t2_tm", 16, 5, 2, tm_in=True, tm_out=True),
    _case("s16_n5_t130_sd5_dest", 16, 5, 130, sd=5.0, layout="dest"),
    _case("s64_n5_t7_bf16_padded", 64, 5, 7, dtype="bf16", padded=True),
    _case("s64_n5_t300_sd5", 64, 5, 300, sd=5.0),
    _case("s64_n5_t65_shift1000", 64, 5, 65, shift=1000.0),
    _case("s64_n5_t65_forbidden_dest", 64, 5, 65, forbidden=True, layout="dest"),
    _case("s256_n5_t1_f16", 256, 5, 1, dtype="f16", out="f16"),
    _case("s256_n5_t65_dest_tm", 256, 5, 65, sd=5.0, layout="dest", tm_in=True, tm_out=True),
    _case("s1024_n3_t2", 1024, 3, 2),
    _case("s1024_n3_t130_f16_dest", 1024, 3, 130, dtype="f16", layout="dest", out="f16"),
    _case("s12_n5_t7_dest_padded", 12, 5, 7, layout="dest", padded=True),
    _case("s12_n5_t130", 12, 5, 130, sd=5.0),
    _case("s8_n9_t2_dest", 8, 9, 2, layout="dest"),
    _case("s8_n9_t65_bf16", 8, 9, 65, dtype="bf16"),
    _case("s80_n9_t7_forbidden", 80, 9, 7, forbidden=True),
    _case("s3_n2_t1_dest", 3, 2, 1, layout="dest"),
    _case("s3_n2_t300_tm", 3, 2, 300, sd=5.0, tm_in=True, tm_out=True),
    _case("s4096_n5_t3_f16", 4096, 5, 3, dtype="f16"),
]
# 8 S + 4608 bytes of LDS per read: S = 8704 is the smallest multiple of 512 that takes the launch past 64 KiB
BIG_LDS = _case("s8704_n3_t2_f16_big_lds", 8704, 3, 2, dtype="f16", out="f16")


def to_bf16_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bf16_bits(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def logz_bound(logz):
    return 2.0 ** -20 * max(1.0, abs(logz))


_built = {}


def build_case(case):
    """-> the case with its inputs and references (computed once and shared: do not modify)"""
    if case["name"] in _built:
        return _built[case["name"]]
    c = dict(case)
    S, N, T = c["S"], c["N"], c["T"]
    B = c["B"] = 3
    rng = np.random.default_rng(1000 + c["seed"] + 7 * S + N + 131 * T)
    lengths = c["lengths"] = np.array([T, max(T - 3, 0), 0], np.int64)
    x = (c["sd"] * rng.standard_normal((B, T, S, N)) + c["shift"]).astype(np.float32)
    if c["forbidden"]:  # a sprinkling of -inf, and one dead state in the last row of every read
        x[rng.random(x.shape) < 0.1] = -np.inf
        for b in range(B):
            if lengths[b]:
                x[b, lengths[b] - 1, S // 2, :] = -np.inf
    # the values the kernel reads, as float32: the reference is computed from the converted values
    if c["dtype"] == "f16":
        stored = x.astype(np.float16)
        x = stored.astype(np.float32)
    elif c["dtype"] == "bf16":
        stored = to_bf16_bits(x)
        x = from_bf16_bits(stored)
    else:
        stored = x
    c["x32"] = x
    if c["layout"] == "dest":
        stored = R.source_to_dest(stored)
    # the array handed over, with the case's strides
    if c["tm_in"]:
        xin = np.ascontiguousarray(stored.transpose(1, 0, 2, 3)).transpose(1, 0, 2, 3)
    elif c["padded"]:
        buf = np.zeros((B, T + 1, S + 1, 2 * N + 1), stored.dtype)
        xin = buf[:, :T, :S, 0:2 * N:2]
        xin[...] = stored
    else:
        xin = np.ascontiguousarray(stored)
    c["xin"] = xin
    c["refs"] = [R.transitions64(x[b, :lengths[b]]) for b in range(B)]
    c["refs32"] = [R.transitions32(x[b, :lengths[b]]) for b in range(B)]
    err = 0.0
    for ref, r32 in zip(c["refs"], c["refs32"]):
        if ref["ok"] and r32["ok"]:
            err = max(err, float(np.abs(r32["init"] - ref["init"]).max()))
            if ref["probs"].size:
                err = max(err, float(np.abs(r32["probs"] - ref["probs"]).max()))
    c["err32"] = err
    _built[case["name"]] = c
    return c


def _half_ulp16(v):
    return np.spacing(np.abs(v).astype(np.float16)).astype(np.float64) / 2


OBSERVED = {}  # case name -> the largest error on p and init the last run_case saw (the figures of INTEGRATION.md 2k)


def check_read(c, b, probs, init, logz, status, where):
    """one read of a result (numpy arrays; probs (T, S, N) of the case's output type) against the float64 reference"""
    ref = c["refs"][b]
    Tr, S, N = int(c["lengths"][b]), c["S"], c["N"]
    assert ref["ok"] and int(status) == 0, where
    tol = 4 * c["err32"] + 2.0 ** -20
    p = probs[:Tr].astype(np.float64)
    half = c["out"] == "f16"
    assert probs.dtype == (np.float16 if half else np.float32)
    assert (probs[Tr:] == SENTINEL).all(), (where, "rows at and beyond T_r were written")
    assert init.dtype == np.float32 and ((init >= 0) & (init <= 1)).all(), where
    worst = float(np.abs(init.astype(np.float64) - ref["init"]).max())
    assert worst <= tol, (where, "init", worst, tol)
    assert abs(float(init.astype(np.float64).sum()) - 1.0) <= S * 2.0 ** -23, (where, "init does not sum to 1")
    assert (init[ref["init"] == 0] == 0).all(), where
    assert abs(logz - ref["logz"]) <= logz_bound(ref["logz"]), (where, "logz", logz, ref["logz"])
    if Tr:
        assert ((p >= 0) & (p <= 1)).all(), where
        allowed = tol + (_half_ulp16(np.maximum(p, ref["probs"])) if half else 0.0)
        d = np.abs(p - ref["probs"])
        assert (d <= allowed).all(), (where, "p", float(d.max()), tol)
        worst = max(worst, float((d - (allowed - tol)).max()))
        live = ref["probs"].sum(axis=2) > 0
        row_tol = N * 2.0 ** -23 + (N * 2.0 ** -12 if half else 0.0)
        assert (np.abs(p.sum(axis=2)[live] - 1.0) <= row_tol).all(), (where, "a live row does not sum to 1")
        assert (p[~live] == 0).all(), (where, "a dead state's row")
        assert (p[np.isneginf(c["x32"][b, :Tr])] == 0).all(), (where, "a forbidden transition has a probability")
    OBSERVED[c["name"]] = max(OBSERVED.get(c["name"], 0.0), worst)


def _device_array(a, device):
    """a numpy array (any strides; uint16 = bfloat16 bits when bf16) -> a torch tensor on `device` with the same strides"""
    import torch
    base = a
    while base.base is not None:
        base = base.base
    flat = torch.from_numpy(np.ascontiguousarray(base).reshape(-1)).to(device)
    off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // a.itemsize
    return torch.as_strided(flat, a.shape, [s // a.itemsize for s in a.strides], off)


def call_abi(fcd, c, device=None, want_logz=True, pad_out=False):
    """The C ABI on the case: sentinel-filled probs with the case's output strides (tm_out: (T, B, S, N); pad_out: spare
    elements between rows and reads) -> probs (B, T, S, N) view, init, logz, status as numpy arrays"""
    from fast_ctc_decode_amd import _native as nat
    B, T, S, N = c["B"], c["T"], c["S"], c["N"]
    xin = c["xin"]
    odt = np.float16 if c["out"] == "f16" else np.float32
    if c["tm_out"]:
        buf = np.full((T, B, S * N + (3 if pad_out else 0)), SENTINEL, odt)
        stride_t, stride_read = buf.strides[0] // buf.itemsize, buf.strides[1] // buf.itemsize
        view = lambda a: a[:, :, :S * N].reshape(T, B, S, N).transpose(1, 0, 2, 3)
    else:
        buf = np.full((B, T + (1 if pad_out else 0), S * N + (3 if pad_out else 0)), SENTINEL, odt)
        stride_read, stride_t = buf.strides[0] // buf.itemsize, buf.strides[1] // buf.itemsize
        view = lambda a: a[:, :T, :S * N].reshape(B, T, S, N)
    stride_read, stride_t = max(stride_read, S * N), max(stride_t, S * N)  # (T = 0: numpy reports no stride)
    init = np.full((B, S + (2 if pad_out else 0)), SENTINEL, np.float32)
    logz = np.full(B, SENTINEL, np.float64)
    status = np.full(B, -1, np.int32)
    st = [s // xin.itemsize for s in xin.strides]
    dcode = {"f32": nat.DTYPE_F32, "f16": nat.DTYPE_F16, "bf16": nat.DTYPE_BF16}[c["dtype"]]
    layout = nat.LAYOUT_DEST if c["layout"] == "dest" else nat.LAYOUT_SOURCE
    if device is None:
        h = nat.default_handle()
        fn = h.lib.fcd_crf_transition_probs_host
        keep = (xin, c["lengths"], buf, init, logz, status)
        ptr = lambda a: a.ctypes.data
    else:
        import torch
        h = nat.default_handle(0)
        fn = h.lib.fcd_crf_transition_probs_dev
        xd = _device_array(xin if c["dtype"] != "bf16" else xin.view(np.int16), device)
        keep = (xd,) + tuple(torch.from_numpy(a).to(device) for a in (c["lengths"], buf, init, logz, status))
        ptr = lambda a: a.data_ptr()
        h.set_stream(torch.cuda.current_stream().cuda_stream)
    b = nat.Batch(ptr(keep[0]), B, T, S, N, st[0], st[1], st[2], st[3], ptr(keep[1]), dcode)
    out = nat.Transitions(ptr(keep[2]), nat.DTYPE_F16 if c["out"] == "f16" else nat.DTYPE_F32, stride_read, stride_t, ptr(keep[3]),
                          init.shape[1], ptr(keep[4]) if want_logz else None, ptr(keep[5]))
    rc = fn(h.ptr, C.byref(b), layout, C.byref(out))
    assert rc == nat.OK, (rc, h.lib.fcd_last_error(h.ptr))
    if device is not None:
        torch.cuda.synchronize()
        buf, init, logz, status = (a.cpu().numpy() for a in keep[2:])
    assert (init[:, S:] == SENTINEL).all()
    return view(buf), init[:, :S], logz, status


def call_api(fcd, c, device=None):
    """crf_transition_probs_batch_raw on the case -> a TransitionResult of numpy arrays"""
    kw = dict(layout=c["layout"], out_dtype="float16" if c["out"] == "f16" else "float32", time_major_out=c["tm_out"])
    if device is None:
        if c["dtype"] == "bf16":
            kw["input_dtype"] = "bfloat16"
        return fcd.crf_transition_probs_batch_raw(c["xin"], c["lengths"], **kw)
    import torch
    xd = _device_array(c["xin"] if c["dtype"] != "bf16" else c["xin"].view(np.int16), device)
    if c["dtype"] == "bf16":
        xd = xd.view(torch.bfloat16)
    r = fcd.crf_transition_probs_batch_raw(xd, torch.from_numpy(c["lengths"]).to(device), **kw)
    assert r.probs.is_cuda and r.init.is_cuda and r.logz.is_cuda and r.status.is_cuda
    return r.cpu()


def run_case(fcd, case, device=None):
    """The C ABI (sentinel rows, the case's strides) against the reference, then the Python function against the C ABI:
    the same bits wherever the call writes.  -> (probs, init, logz, status) of the C ABI call"""
    c = build_case(case)
    probs, init, logz, status = call_abi(fcd, c, device)
    for b in range(c["B"]):
        check_read(c, b, probs[b], init[b], float(logz[b]), status[b], (c["name"], b))
    Tr0 = int(c["lengths"][2])
    assert Tr0 == 0 and np.array_equal(init[2], np.full(c["S"], np.float32(1) / np.float32(c["S"]))) and logz[2] == np.log(float(c["S"]))
    r = call_api(fcd, c, device)
    assert r.probs.shape == probs.shape and r.probs.dtype == probs.dtype
    for b in range(c["B"]):
        n = int(c["lengths"][b])
        assert np.array_equal(r.probs[b, :n], probs[b, :n]), (c["name"], b, "the Python function and the C ABI differ")
    assert np.array_equal(r.init, init) and np.array_equal(r.logz, logz) and np.array_equal(r.status, status)
    return probs, init, logz, status


def _conv(device):
    if device is None:
        return lambda a: a
    import torch
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)


def edge_cases(fcd, device=None):
    """a NaN row, a +inf, a row nothing passes, T_r = 0, and failed reads beside good ones"""
    to = _conv(device)
    rng = np.random.default_rng(17)
    for S, N, T in ((4, 5, 9), (64, 5, 6), (256, 3, 5)):
        good = R.random_scores(rng, T, S, N)
        x = np.stack([good] * 6)
        x[1, 2] = np.nan                   # a NaN row
        x[2, T - 1, S - 1, N - 1] = np.inf  # one +inf
        x[3, 1] = -np.inf                  # a row nothing passes: no path has positive weight
        x[4, 0, 0, 0] = np.nan             # ... beyond the read's length: not looked at
        lengths = np.array([T, T, T, T, 0, T], np.int64)
        r = fcd.crf_transition_probs_batch_raw(to(x), to(lengths)).cpu()
        solo = fcd.crf_transition_probs_batch_raw(to(good[None])).cpu()
        assert r.status.tolist() == [0, 2, 2, 2, 0, 0], (S, r.status)
        assert np.isnan(r.logz[1:4]).all() and r.logz[4] == np.log(float(S))
        assert np.array_equal(r.init[4], np.full(S, np.float32(1) / np.float32(S)))
        for b in (0, 5):  # the good reads are what they are on their own
            assert np.array_equal(r.probs[b], solo.probs[0]) and np.array_equal(r.init[b], solo.init[0]) and r.logz[b] == solo.logz[0]
        ref = R.transitions64(good)
        assert abs(r.logz[0] - ref["logz"]) <= logz_bound(ref["logz"])
        # a -inf score alone fails nothing: its transition has probability exactly 0, a dead state's row is zeros
        y = good.copy()
        y[T - 2, 1, :] = -np.inf
        y[0, 2, 1] = -np.inf
        y[0, 3, :] = -np.inf  # dead at row 0: init 0
        d = fcd.crf_transition_probs_batch_raw(to(y[None])).cpu()
        assert int(d.status[0]) == 0 and (d.probs[0, T - 2, 1] == 0).all() and d.probs[0, 0, 2, 1] == 0 and d.init[0, 3] == 0
        assert (d.probs[0, 0, 3] == 0).all()
        ref = R.transitions64(y)
        assert np.abs(d.probs[0] - ref["probs"]).max() < 1e-5 and abs(d.logz[0] - ref["logz"]) <= logz_bound(ref["logz"])
    # the single-read function raises with the status string
    import pytest
    if device is None:
        probs, init, logz = fcd.crf_transition_probs(good)
        assert probs.shape == good.shape and init.shape == (good.shape[1],) and isinstance(logz, float)
        assert np.array_equal(probs, solo.probs[0]) and logz == solo.logz[0]
        pd, idd, lzd = fcd.crf_transition_probs(R.source_to_dest(good), layout="dest")
        assert np.array_equal(pd, probs) and np.array_equal(idd, init) and lzd == logz
        with pytest.raises(RuntimeError, match="Failed to compare values"):
            fcd.crf_transition_probs(x[1])


def nullable_outputs(fcd, device=None):
    """out->logz is nullable: the other outputs are the same bits with and without it; spare elements between rows, reads
    and init rows stay untouched"""
    c = build_case([k for k in CASES if k["name"] == "s16_n5_t130_sd5_dest"][0])
    full = call_abi(fcd, c, device)
    for want_logz, pad_out in ((False, False), (True, True), (False, True)):
        got = call_abi(fcd, c, device, want_logz=want_logz, pad_out=pad_out)
        for b in range(c["B"]):
            n = int(c["lengths"][b])
            assert np.array_equal(got[0][b, :n], full[0][b, :n]) and (got[0][b, n:] == SENTINEL).all()
        assert np.array_equal(got[1], full[1]) and np.array_equal(got[3], full[3])
        assert np.array_equal(got[2], full[2]) if want_logz else (got[2] == SENTINEL).all()


def argument_errors(fcd, device=None):
    """the argument errors at both layers, and every limit"""
    import pytest
    from fast_ctc_decode_amd import _native as nat
    to = _conv(device)
    x = R.random_scores(np.random.default_rng(3), 6, 4, 5)
    xb = to(x[None])
    with pytest.raises(ValueError, match="layout"):
        fcd.crf_transition_probs_batch_raw(xb, layout="both")
    with pytest.raises(ValueError, match="out_dtype"):
        fcd.crf_transition_probs_batch_raw(xb, out_dtype="bfloat16")
    with pytest.raises(ValueError, match="lengths must have shape"):
        fcd.crf_transition_probs_batch_raw(xb, to(np.array([1, 2], np.int64)))
    with pytest.raises(TypeError):
        fcd.crf_transition_probs_batch_raw(to(x))  # rank 3
    if device is None:
        with pytest.raises(TypeError):
            fcd.crf_transition_probs_batch_raw(x.astype(np.float64)[None])
        with pytest.raises(TypeError):
            fcd.crf_transition_probs(x[None])  # rank 4

    def wide(shape):  # one element seen as a large array: the limits are refused before anything is read
        if device is None:
            return np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape, (0, 0, 0, 0))
        import torch
        return torch.zeros(1, device=device).expand(shape)
    for shape, words in (((1, 2, 5, 4), "multiple of N - 1"), ((1, 2, 9, 10), "2 .. 9"), ((1, 2, 4, 1), "2 .. 9"),
                         ((1, 1, 1 << 24, 2), "below 2^24"), ((1, 1, 20480, 3), "LDS")):
        with pytest.raises(nat.NativeError) as e:
            fcd.crf_transition_probs_batch_raw(wide(shape))
        assert e.value.code == nat.E_UNSUPPORTED and "crf_transition_probs" in str(e.value) and words in str(e.value), shape
    r = fcd.crf_transition_probs_batch_raw(wide((1, 1, 19904, 3))).cpu()  # the largest S the LDS holds
    assert int(r.status[0]) == 0 and abs(float(r.probs[0, 0].sum()) - 19904) < 1e-2 and abs(r.logz[0] - np.log(3 * 19904.0)) < 1e-5
    # the C ABI itself
    h = nat.default_handle() if device is None else nat.default_handle(0)
    fn = h.lib.fcd_crf_transition_probs_host if device is None else h.lib.fcd_crf_transition_probs_dev
    if device is None:
        keep = [x, np.zeros((6, 4, 5), np.float32), np.zeros(4, np.float32), np.zeros(1), np.zeros(1, np.int32)]
        ptr = lambda a: a.ctypes.data
    else:
        import torch
        keep = [torch.from_numpy(a).to(device) for a in (x, np.zeros((6, 4, 5), np.float32), np.zeros(4, np.float32), np.zeros(1),
                                                         np.zeros(1, np.int32))]
        ptr = lambda a: a.data_ptr()
    xp, pp, ip, zp, sp = (ptr(a) for a in keep)
    b = nat.Batch(xp, 1, 6, 4, 5, 120, 20, 5, 1, None)

    def tr(probs=pp, dtype=nat.DTYPE_F32, stride_read=120, stride_t=20, init=ip, init_stride=4, logz=zp, status=sp):
        return nat.Transitions(probs, dtype, stride_read, stride_t, init, init_stride, logz, status)
    assert fn(h.ptr, C.byref(b), 0, C.byref(tr())) == nat.OK
    assert fn(h.ptr, None, 0, C.byref(tr())) == nat.E_INVALID
    assert fn(h.ptr, C.byref(b), 0, None) == nat.E_INVALID
    for bad in (tr(probs=None), tr(init=None), tr(status=None), tr(dtype=nat.DTYPE_BF16), tr(dtype=7), tr(stride_read=19),
                tr(stride_t=19), tr(init_stride=3)):
        assert fn(h.ptr, C.byref(b), 0, C.byref(bad)) == nat.E_INVALID
    for layout in (-1, 2):
        assert fn(h.ptr, C.byref(b), layout, C.byref(tr())) == nat.E_INVALID
    assert fn(h.ptr, C.byref(nat.Batch(None, 1, 6, 4, 5, 120, 20, 5, 1, None)), 0, C.byref(tr())) == nat.E_INVALID  # null scores
    bad_dtype = nat.Batch(xp, 1, 6, 4, 5, 120, 20, 5, 1, None, 9)
    assert fn(h.ptr, C.byref(bad_dtype), 0, C.byref(tr())) == nat.E_INVALID
    assert fn(h.ptr, C.byref(nat.Batch(xp, 1, 6, 4, 5, 120, -20, 5, 1, None)), 0, C.byref(tr())) == nat.E_INVALID
    empty = nat.Batch(None, 0, 6, 4, 5, 120, 20, 5, 1, None)
    assert fn(h.ptr, C.byref(empty), 0, C.byref(tr(probs=None, init=None, status=None))) == nat.OK  # no reads: nothing to do


def peaked_scores(rng, B, T, S, N, gap=6.0):
    """scores whose best path is unambiguous in float32: N(0, 1) noise, and along one random path per read a bonus of `gap`"""
    x = rng.standard_normal((B, T, S, N)).astype(np.float32)
    d = R.destinations(S, N)
    for b in range(B):
        s = int(rng.integers(S))
        for t in range(T):
            a = int(rng.integers(N))
            x[b, t, s, a] += gap
            s = int(d[s, a])
    return x


def best_path64(x):
    """float64 Viterbi over the scores: max over start states and symbol sequences of the score sum -> (score, s0, emitting rows, labels)"""
    T, S, N = x.shape
    d = R.destinations(S, N)
    v = np.zeros(S)
    arg = np.zeros((T, S), np.int64)
    for t in range(T - 1, -1, -1):
        y = x[t].astype(np.float64) + v[d]
        arg[t] = y.argmax(axis=1)
        v = y.max(axis=1)
    s0 = s = int(v.argmax())
    rows, labels = [], []
    for t in range(T):
        a = int(arg[t, s])
        if a:
            rows.append(t)
            labels.append(a)
        s = int(d[s, a])
    return float(v.max()), s0, rows, labels
