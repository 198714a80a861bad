"""TEST INFRASTRUCTURE shared by tests/test_ctc_align_emu.py (the kernels on the wave64 emulator) and
tests/test_gpu_ctc_align.py (on the GPU): the shape grid of tests/ctc_score_cases.py run through ctc_align_batch_raw and
compared with the restatement tests/ctc_align_reference.py, and the greedy-parity check against viterbi_search.

start, count and qual must equal the restatement EXACTLY (the kernel's arithmetic is the restatement's: f32 mantissa
products, exact rescaling, the same tie rule); logp within 1e-12 relative (ln(m 2^k) against ln m + k ln 2 in float64).
Condition on the inputs, asserted for every labelling: the restatement with drop=2^-160 returns the same alignment -- no
case relies on cells the contract lets the kernel drop.
Properties: spans disjoint, ascending, count >= 1; the float64 product of the posteriors along the returned alignment is
logp within 2 T_r 2^-24 (one f32 rounding per row); logp <= ctc_score + 2 tolerance at the same band; band W <= band 2W
<= exact in logp, with no slack beyond the 1e-12 relative of the float64 tail: max and a single rounding are monotone and
the rescaling is exact, so every cell of a wider window is at least the same cell of the narrower one."""
import math

import numpy as np

import ctc_align_reference as A
import ctc_score_cases as SC


def logp_same(got, want):
    if want != want:
        return got != got
    if math.isinf(want):
        return got == want
    return abs(got - want) <= 1e-12 * max(1.0, abs(want))


def check(got, x32, lengths, labels, paths, out_len, n_valid, collapse, band, rows=None):
    """got: AlignResult of numpy arrays; x32: the posteriors as float32 (the exact upcast of what the kernel read).
    -> {(b, i): restatement result} of the labellings compared."""
    B, n_hyp = got.logp.shape
    refs = {}
    for b in (range(B) if rows is None else rows):
        Tr = x32.shape[1] if lengths is None else int(lengths[b])
        for i in range(n_hyp):
            n = int(out_len[b, i])
            if n_valid is not None and i >= int(n_valid[b]):
                assert got.logp[b, i] != got.logp[b, i], ("rows that are no hypothesis are NaN", b, i)
                assert (got.count[b, i, :min(n, labels.shape[2])] == 0).all()
                continue
            y, pth = labels[b, i, :n], (paths[b, i, :n] if band else None)
            ref = A.ctc_align(x32[b, :Tr], y, collapse, band, pth)
            cond = A.ctc_align(x32[b, :Tr], y, collapse, band, pth, drop=2.0 ** -160)
            assert ref["states"] == cond["states"], ("the case relies on dropped cells", b, i)
            where = (b, i, "T_r", Tr, "L", n, "band", band)
            assert logp_same(got.logp[b, i], ref["logp"]), where + (got.logp[b, i], ref["logp"])
            refs[(b, i)] = ref
            if ref["states"] is None:
                assert (got.count[b, i, :n] == 0).all(), where
                continue
            assert got.start[b, i, :n].tolist() == ref["start"], where
            assert got.count[b, i, :n].tolist() == ref["count"], where
            assert got.qual[b, i, :n].view(np.uint32).tolist() == np.asarray(ref["qual"], np.float32).view(np.uint32).tolist(), where
            # properties
            st, ct = got.start[b, i, :n].astype(np.int64), got.count[b, i, :n].astype(np.int64)
            assert (ct >= 1).all() and (collapse or (ct == 1).all()), where
            assert (st[1:] >= st[:-1] + ct[:-1]).all() and (n == 0 or st[-1] + ct[-1] <= Tr), where
            z = [0] * (2 * n + 1)
            z[1::2] = [int(v) for v in y]
            prod = sum(math.log(float(x32[b, t, z[s]])) for t, s in enumerate(ref["states"]))
            assert abs(prod - got.logp[b, i]) <= 2 * Tr * 2.0 ** -24, where + (prod, got.logp[b, i])
    return refs


def host_abi_optional_pointers(fcd, S=None):
    """fcd_ctc_align_host (S None) / fcd_crf_align_host (S states) through ctypes, at every combination of the pointers the
    C ABI makes optional: lengths and n_valid null or given, band 0 without path and band 2 with it, and qual / logp null
    singly and together -- on time-major posteriors, B = 3, T = 7, N = 5, two hypotheses in rows of 8.  The call with
    qual and logp goes through check() (the restatement); a call without one of them must give the other arrays bit for
    bit and leave nothing else written.  Entries k >= len come back 0, whatever the caller's arrays held."""
    import ctypes as C
    import itertools
    from types import SimpleNamespace
    from fast_ctc_decode_amd import _native as nat
    B, T, N, n_hyp, stride = 3, 7, 5, 2, 8
    rng = np.random.default_rng(31 + (S or 0))
    if S is None:
        x, init, row = SC.posteriors(rng, B, T, N), None, N
    else:
        import crf_lattice_cases as CC
        x, init, row = CC.posteriors(rng, B, T, S, N), rng.random((B, S)).astype(np.float32), S * N
    xt = np.ascontiguousarray(np.moveaxis(x, 0, 1))  # (T, B, ..): reads are `row` elements apart, rows B * row
    lengths, n_valid = np.array([T, 4, 6], np.int64), np.array([2, 1, 2], np.uint32)
    labels, paths = np.zeros((B, n_hyp, stride), np.uint8), np.zeros((B, n_hyp, stride), np.uint32)
    lens = np.zeros((B, n_hyp), np.uint32)
    for b in range(B):
        for i in range(n_hyp):
            L = 1 + (b + i) % 3
            labels[b, i, :L] = [1 + (k + b + i) % (N - 1) for k in range(L)]  # (neighbours differ: L rows do)
            paths[b, i, :L] = np.sort(rng.choice(4, L, replace=False))        # (inside the shortest read)
            lens[b, i] = L
    h = nat.default_handle()

    def run(with_len, with_nv, band, qual=True, logp=True):
        r = SimpleNamespace(start=np.full((B, n_hyp, stride), 77, np.uint32), count=np.full((B, n_hyp, stride), 77, np.uint32),
                            qual=np.full((B, n_hyp, stride), 77.0, np.float32), logp=np.full((B, n_hyp), 77.0))
        b_ = nat.Batch(xt.ctypes.data, B, T, S or 1, N, row, B * row, 0 if S is None else N, 1,
                       lengths.ctypes.data if with_len else None)
        y_ = nat.Labellings(labels.ctypes.data, lens.ctypes.data, n_valid.ctypes.data if with_nv else None,
                            paths.ctypes.data if band else None, n_hyp, stride)
        out = nat.Alignment(r.start.ctypes.data, r.count.ctypes.data, r.qual.ctypes.data if qual else None,
                            r.logp.ctypes.data if logp else None)
        if S is None:
            rc = h.lib.fcd_ctc_align_host(h.ptr, C.byref(b_), C.byref(y_), 1, band, C.byref(out))
        else:
            rc = h.lib.fcd_crf_align_host(h.ptr, C.byref(b_), init.ctypes.data, S, S, C.byref(y_), band, C.byref(out))
        assert rc == nat.OK, h.lib.fcd_last_error(h.ptr)
        return r

    for with_len, with_nv, band in itertools.product((False, True), (False, True), (0, 2)):
        where = (with_len, with_nv, band)
        full = run(with_len, with_nv, band)
        ls, nv = lengths if with_len else None, n_valid if with_nv else None
        if S is None:
            check(full, x, ls, labels, paths, lens, nv, True, band)
        else:
            CC.check(full, None, x, init, ls, labels, paths, lens, nv, band)
        assert np.isfinite(full.logp[:, 0]).all() and (full.count[:, 0, 0] >= 1).all(), where  # (alignments, not refusals)
        for b in range(B):
            for i in range(n_hyp):
                n = int(lens[b, i])
                assert not full.start[b, i, n:].any() and not full.count[b, i, n:].any() and not full.qual[b, i, n:].any(), where
        for qual, logp in ((False, True), (True, False), (False, False)):
            part = run(with_len, with_nv, band, qual, logp)
            assert np.array_equal(part.start, full.start) and np.array_equal(part.count, full.count), where + (qual, logp)
            assert np.array_equal(part.qual.view(np.uint32), full.qual.view(np.uint32)) if qual else (part.qual == 77).all()
            assert np.array_equal(part.logp, full.logp, equal_nan=True) if logp else (part.logp == 77).all()


def _device_inputs(c, device):
    """(xin, conv, kw) of a ctc_score_cases case for numpy (device None) or torch tensors on `device`"""
    kw = {}
    if device is None:
        if c["dtype"] == "bf16":
            kw["input_dtype"] = "bfloat16"
        return c["xin"], (lambda a: a), kw
    import torch
    if c["dtype"] == "bf16":
        xin = torch.from_numpy(np.ascontiguousarray(c["xin"]).view(np.int16)).to(device).view(torch.bfloat16)
    else:
        xin = torch.from_numpy(np.ascontiguousarray(c["xin"])).to(device)
    if c["xin"].strides[0] < c["xin"].strides[1]:  # time-major on the device too
        xin = xin.transpose(0, 1).contiguous().transpose(0, 1)
    conv = lambda a: None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device)
    return xin, conv, kw


def run_case(fcd, c, device=None):
    """aligns the case at each of its bands, checks every labelling against the restatement, then the properties that
    tie the bands to one another and to ctc_score"""
    xin, conv, kw = _device_inputs(c, device)
    by_band = {}
    for band in c["bands"]:
        args = (xin, conv(c["labels"]), conv(c["out_len"]), c["collapse"], conv(c["lengths"]),
                conv(c["paths"]) if band else None, band, conv(c["n_valid"]))
        got = fcd.ctc_align_batch_raw(*args, **kw)
        score = fcd.ctc_score_batch_raw(*args, **kw)
        if device is not None:
            import torch
            assert got.start.device == xin.device and got.logp.dtype == torch.float64
            score = score.cpu().numpy()
        got = got.cpu()
        assert got.start.shape == c["labels"].shape and got.count.shape == c["labels"].shape
        assert got.qual.shape == c["labels"].shape and got.logp.shape == c["out_len"].shape
        assert got.start.dtype == np.uint32 and got.qual.dtype == np.float32 and got.logp.dtype == np.float64
        refs = check(got, c["x32"], c["lengths"], c["labels"], c["paths"], c["out_len"], c["n_valid"], c["collapse"], band)
        for (b, i) in refs:  # one alignment is no more than all of them
            Tr = c["T"] if c["lengths"] is None else int(c["lengths"][b])
            if got.logp[b, i] == got.logp[b, i]:
                assert got.logp[b, i] <= score[b, i] + 2 * SC.tolerance(Tr), (c["name"], band, b, i, got.logp[b, i], score[b, i])
        by_band[band] = refs, got.logp
    order = sorted(b for b in by_band if b) + ([0] if 0 in by_band else [])
    for lo_b, hi_b in zip(order, order[1:]):
        g_lo, g_hi = by_band[lo_b][1], by_band[hi_b][1]
        for (b, i) in by_band[lo_b][0]:
            if g_lo[b, i] == g_lo[b, i] and g_hi[b, i] == g_hi[b, i]:
                assert g_lo[b, i] <= g_hi[b, i] or (math.isfinite(g_hi[b, i]) and
                                                    g_lo[b, i] - g_hi[b, i] <= 1e-12 * max(1.0, abs(g_hi[b, i]))), \
                    (c["name"], b, i, lo_b, hi_b, g_lo[b, i], g_hi[b, i])  # (-inf <= -inf: no arithmetic on infinities)
    return by_band


def greedy_posteriors(rng, B, T, N, margin=1.05):
    """posteriors whose largest entry of every row is at least `margin` times the second: the maximum of a row that
    falls short is boosted and the row renormalised.  float32."""
    x = SC.posteriors(rng, B, T, N, sharp=1.5).astype(np.float64)
    top = x.argmax(-1)
    srt = np.sort(x, -1)
    short = srt[..., -1] < 1.2 * margin * srt[..., -2]
    boost = np.where(short, 1.2 * margin * srt[..., -2], srt[..., -1])
    np.put_along_axis(x, top[..., None], boost[..., None], -1)
    return (x / x.sum(-1, keepdims=True)).astype(np.float32)


def greedy_parity(fcd, T, dtype, device=None, collapse=True):
    """aligning viterbi_search's own labelling gives back its path and its qualities bit for bit"""
    B, N = 8, 5
    rng = np.random.default_rng(1000 + T + (dtype == "f16"))
    x = greedy_posteriors(rng, B, T, N)
    if dtype == "f16":
        x = x.astype(np.float16)
    x32 = x.astype(np.float32)
    srt = np.sort(x32.astype(np.float64), -1)
    assert (srt[..., -1] >= 1.05 * srt[..., -2]).all()  # (on the array the kernels read: no read is excluded)
    lengths = rng.integers(max(1, T // 2), T + 1, size=B).astype(np.int64)
    lengths[0] = T
    if device is None:
        xin, lin = x, lengths
    else:
        import torch
        xin, lin = torch.from_numpy(x).to(device), torch.from_numpy(lengths).to(device)
    r = fcd.viterbi_search_batch_raw(xin, collapse, lin, qual=True)
    rc = r.cpu()
    for band in (0, 4):
        got = fcd.ctc_align_batch_raw(xin, r.labels, r.out_len, collapse, lin, r.path if band else None, band).cpu()
        for b in range(B):
            Tr, n = int(lengths[b]), int(rc.out_len[b])
            lab = x32[b, :Tr].argmax(-1)
            assert got.start[b, 0, :n].tolist() == np.asarray(rc.path[b, :n]).astype(np.uint32).tolist(), (T, dtype, band, b)
            assert got.qual[b, 0, :n].view(np.uint32).tolist() == np.asarray(rc.qual[b, :n]).view(np.uint32).tolist(), (T, dtype, band, b)
            runs = []  # run lengths of the greedy labels, recomputed: a new run at every emission
            for t in range(Tr):
                if lab[t] != 0 and (not collapse or t == 0 or lab[t - 1] != lab[t]):
                    runs.append(1)
                elif lab[t] != 0:
                    runs[-1] += 1
            assert len(runs) == n and got.count[b, 0, :n].tolist() == runs, (T, dtype, band, b)
            want = np.log(x32[b, :Tr].max(-1).astype(np.float64)).sum()
            assert abs(got.logp[b, 0] - want) <= 2 * T * 2.0 ** -24, (T, dtype, band, b, got.logp[b, 0], want)


def wide_window_parity(fcd, device="cuda"):
    """The LDS kernel with more than 16 x 1024 live states in a row, so that its work-items hold cells 16 .. 19 of their
    20: exact mode, T = 16750 rows, about 8400 labels (every non-blank row emits: collapse_repeats = 0), where the
    window of the middle rows is 2 min(L, T - L) + 1 > 16384 states wide.  Read 0 emits all its labels in the first half
    (the alignment runs along the window's upper edge there: cells 16 and up), read 1 in the second half (the lower
    edge: cell 0, whose back-pointer shares a word with cell 16's).  Every row's maximum is 6 times its second, so the
    greedy path is the best alignment: start, count and qual must be viterbi_search's."""
    import torch
    T, N, half = 16750, 5, 8400
    rng = np.random.default_rng(77)
    sym = np.zeros((2, T), np.int64)
    sym[0, :half] = rng.integers(1, N, half)
    sym[1, T - half:] = rng.integers(1, N, half)
    for b, sl in ((0, slice(0, half)), (1, slice(T - half, T))):  # a few blanks inside the label half
        sym[b, sl][rng.choice(half, 40, replace=False)] = 0
    x = np.full((2, T, N), 0.1, np.float32)
    np.put_along_axis(x, sym[..., None], np.float32(0.6), -1)
    x *= (1.0 + 0.01 * rng.random((2, T, 1))).astype(np.float32)  # (rows differ; the margin within a row stays 6)
    xd = torch.from_numpy(x).to(device)
    r = fcd.viterbi_search_batch_raw(xd, False, None, qual=True)
    rc = r.cpu()
    stride = 8500  # (2 * 8500 + 1 states: what the 160 KiB of LDS hold)
    L = np.asarray(rc.out_len).astype(np.int64)
    assert (L == half - 40).all() and (2 * np.minimum(L, T - L) + 1 > 16 * 1024).all() and (L <= stride).all()
    got = fcd.ctc_align_batch_raw(xd, r.labels[:, :stride].contiguous(), r.out_len, False).cpu()
    for b in range(2):
        n = int(L[b])
        assert got.start[b, 0, :n].tolist() == np.asarray(rc.path[b, :n]).astype(np.uint32).tolist(), b
        assert (got.count[b, 0, :n] == 1).all(), b
        assert got.qual[b, 0, :n].view(np.uint32).tolist() == np.asarray(rc.qual[b, :n]).view(np.uint32).tolist(), b
        want = np.log(x[b].max(-1).astype(np.float64)).sum()
        assert abs(got.logp[b, 0] - want) <= 2 * T * 2.0 ** -24, (b, got.logp[b, 0], want)
