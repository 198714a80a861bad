"""TEST INFRASTRUCTURE shared by tests/test_ctc_score_emu.py (the kernels on the wave64 emulator) and
tests/test_gpu_ctc_score.py (on the GPU): inputs, hypotheses and the comparison of ctc_score_batch_raw with the float64
restatement tests/ctc_score_reference.py.

Tolerance: |logp - ref| <= 4 * T_r * 2^-24 nats.  Per cell and step the kernel rounds at most three times in f32 (two
additions, one product), every term is non-negative, the rescaling is by exact powers of two and the tail is float64:
the relative error of P is at most 3 * T * 2^-24 to first order; the factor 4 leaves room for the second-order term.
Condition on the inputs, checked for every labelling: zeroing the cells below 2^-160 of their row's maximum changes the
restatement by less than 1e-9 -- no case relies on mass the contract lets the kernel drop."""
import math

import numpy as np

import ctc_score_reference as R


def posteriors(rng, B, T, N, sharp=2.5):
    """softmax rows floored at 1e-4 and renormalised, float32"""
    x = np.exp(rng.standard_normal((B, T, N)) * sharp)
    x = x / x.sum(-1, keepdims=True)
    x = np.maximum(x, 1e-4)
    return (x / x.sum(-1, keepdims=True)).astype(np.float32)


def to_f16(x):
    return x.astype(np.float16)


def to_bf16_bits(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_bits_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def edit(rng, labels, path, N, T):
    """a random substitution, deletion or insertion (a repeat of the neighbour half of the time); the path stays
    ascending (an inserted label takes its successor's row)"""
    labels, path = list(labels), list(path)
    kind = rng.integers(3) if labels else 2
    if kind == 0:
        labels[rng.integers(len(labels))] = int(rng.integers(1, N))
    elif kind == 1:
        i = int(rng.integers(len(labels)))
        del labels[i], path[i]
    else:
        i = int(rng.integers(len(labels) + 1))
        row = path[i] if i < len(path) else max(T - 1, 0)
        lab = labels[i - 1] if (i > 0 and rng.integers(2)) else int(rng.integers(1, N))
        labels.insert(i, lab)
        path.insert(i, row)
    return labels, path


def hypotheses(fcd, rng, x, lengths, n_hyp, collapse, n_edits=2):
    """(labels (B, n_hyp, T) u8, paths u32, out_len (B, n_hyp) u32, n_valid (B,) u32): the n best of the beam search
    on the batch; every second labelling then takes up to n_edits random edits.  x: float32 / float16 numpy."""
    B, T, N = x.shape
    r = fcd.beam_search_nbest_batch_raw(x, n_hyp, beam_size=max(5, n_hyp), collapse_repeats=collapse, lengths=lengths)
    labels, paths, out_len = r.labels.copy(), r.path.copy(), r.out_len.copy()
    n_valid = np.asarray(r.n_hyp, np.uint32).copy()
    for b in range(B):
        Tr = T if lengths is None else int(lengths[b])
        for i in range(int(n_valid[b])):
            if (b + i) % 2 == 0:
                continue
            n = int(out_len[b, i])
            lab, pth = labels[b, i, :n].tolist(), paths[b, i, :n].tolist()
            for _ in range(int(rng.integers(1, n_edits + 1))):
                lab, pth = edit(rng, lab, pth, N, Tr)
            if len(lab) > labels.shape[2]:
                continue
            labels[b, i] = 0
            paths[b, i] = 0
            labels[b, i, :len(lab)] = lab
            paths[b, i, :len(lab)] = pth
            out_len[b, i] = len(lab)
    return labels, paths, out_len, n_valid


def tolerance(Tr):
    return 4.0 * max(Tr, 1) * 2.0 ** -24


def same(got, want, Tr):
    if want != want:
        return got != got
    if math.isinf(want):
        return got == want
    return abs(got - want) <= tolerance(Tr)


def check(got, x32, lengths, labels, paths, out_len, n_valid, collapse, band, rows=None, verbose=False):
    """got: (B, n_hyp) float64 from the kernel; x32: the posteriors as float32 (the exact upcast of what the kernel
    read).  rows: the reads to compare (default all).  Returns the reference values it computed, {(b, i): ref}."""
    got = np.asarray(got)
    B, n_hyp = got.shape
    refs = {}
    worst = 0.0
    for b in (range(B) if rows is None else rows):
        Tr = x32.shape[1] if lengths is None else int(lengths[b])
        for i in range(n_hyp):
            if n_valid is not None and i >= int(n_valid[b]):
                assert got[b, i] != got[b, i], ("unscored rows are NaN", b, i, got[b, i])
                continue
            n = int(out_len[b, i])
            y, pth = labels[b, i, :n], (paths[b, i, :n] if band else None)
            ref = R.ctc_logp(x32[b, :Tr], y, collapse, band, pth)
            cond = R.ctc_logp(x32[b, :Tr], y, collapse, band, pth, drop=2.0 ** -160)
            assert (ref == cond) or abs(ref - cond) <= 1e-9, ("the case relies on dropped mass", b, i, ref, cond)
            if verbose and ref == ref and not math.isinf(ref):
                worst = max(worst, abs(got[b, i] - ref) / tolerance(Tr))
            assert same(got[b, i], ref, Tr), (b, i, "T_r", Tr, "L", n, "band", band, got[b, i], ref,
                                              abs(got[b, i] - ref), tolerance(Tr))
            refs[(b, i)] = ref
    if verbose:
        print("ctc_score: band %d, %d labellings, worst |error| / tolerance = %.3f" % (band, len(refs), worst))
    return refs


# (name, N, T, B, n_hyp, dtype, time_major, collapse, ragged, bands)  -- bands: 0 = exact
#   window sizes: exact 2 min(T, stride) + 1 states, banded min(that, 4 W + 3); up to 510 states live in registers
#   (2 / 4 / 6 / 8 per lane at 126 / 254 / 382 / 510), more in LDS
CASES = [
    ("n2-tiny", 2, 9, 5, 2, "f32", False, True, True, (0, 1, 4)),
    ("n5-regs2", 5, 40, 6, 3, "f32", False, True, True, (0, 1, 4, 64)),
    ("n5-nocollapse", 5, 60, 4, 5, "f32", False, False, True, (0, 1, 4, 64)),
    ("n5-regs4-f16", 5, 110, 3, 2, "f16", False, True, False, (0, 4, 16)),
    ("n7-regs6-bf16", 7, 170, 2, 2, "bf16", False, True, True, (0, 4, 64)),
    ("n4-regs8-timemajor", 4, 230, 3, 1, "f32", True, True, True, (0, 1, 64)),
    ("n12-lds", 12, 300, 3, 2, "f32", False, True, True, (0, 1, 4, 64, 128)),
    ("n5-lds-nocollapse-timemajor-f16", 5, 280, 2, 3, "f16", True, False, False, (0, 128)),
]


def build_case(fcd, case):
    name, N, T, B, n_hyp, dtype, time_major, collapse, ragged, bands = case
    rng = np.random.default_rng(sum(map(ord, name)))
    x = posteriors(rng, B, T, N)
    lengths = None
    if ragged:
        lengths = rng.integers(max(1, T // 2), T + 1, size=B).astype(np.int64)
        lengths[0] = T
        if B > 2:
            lengths[1] = 1
    if dtype == "f16":
        xin = to_f16(x)
        x32 = xin.astype(np.float32)
    elif dtype == "bf16":
        xin = to_bf16_bits(x)
        x32 = bf16_bits_to_f32(xin)
    else:
        xin, x32 = x, x
    labels, paths, out_len, n_valid = hypotheses(fcd, rng, x32 if dtype == "bf16" else xin, lengths, n_hyp, collapse)
    if time_major:  # the (T, B, N) tensor a network emits, seen as a batch
        xin = np.ascontiguousarray(xin.transpose(1, 0, 2)).transpose(1, 0, 2)
    return dict(name=name, xin=xin, x32=x32, lengths=lengths, labels=labels, paths=paths, out_len=out_len,
                n_valid=n_valid, collapse=collapse, bands=bands, dtype=dtype, N=N, T=T)


def run_case(fcd, c, device=None, verbose=False):
    """scores the case at each of its bands (numpy through _host, or torch tensors on `device` through _dev), checks
    every value against the restatement and band W <= band 2W <= exact within the tolerance"""
    kw = {}
    if device is None:
        xin = c["xin"]
        if c["dtype"] == "bf16":
            kw["input_dtype"] = "bfloat16"
        conv = lambda a: a
    else:
        import torch
        if c["dtype"] == "bf16":
            base = c["xin"]
            t = torch.from_numpy(np.ascontiguousarray(base).view(np.int16)).to(device).view(torch.bfloat16)
            xin = t
        else:
            xin = torch.from_numpy(np.ascontiguousarray(c["xin"])).to(device)
        if c["xin"].strides[0] < c["xin"].strides[1]:  # time-major on the device too
            xin = xin.transpose(0, 1).contiguous().transpose(0, 1)
        conv = lambda a: None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device)
    by_band = {}
    for band in c["bands"]:
        got = fcd.ctc_score_batch_raw(xin, conv(c["labels"]), conv(c["out_len"]), c["collapse"], conv(c["lengths"]),
                                      conv(c["paths"]) if band else None, band, conv(c["n_valid"]), **kw)
        if device is not None:
            assert got.dtype == __import__("torch").float64 and got.device == xin.device
            got = got.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == c["out_len"].shape
        by_band[band] = check(got, c["x32"], c["lengths"], c["labels"], c["paths"], c["out_len"], c["n_valid"],
                              c["collapse"], band, verbose=verbose), got
    # properties: a band is a lower bound that rises with W
    order = sorted(b for b in by_band if b) + ([0] if 0 in by_band else [])
    for lo_b, hi_b in zip(order, order[1:]):
        g_lo, g_hi = by_band[lo_b][1], by_band[hi_b][1]
        for (b, i) in by_band[lo_b][0]:
            Tr = c["T"] if c["lengths"] is None else int(c["lengths"][b])
            if g_lo[b, i] == g_lo[b, i] and g_hi[b, i] == g_hi[b, i]:
                assert g_lo[b, i] <= g_hi[b, i] + 2 * tolerance(Tr), (c["name"], b, i, lo_b, hi_b, g_lo[b, i], g_hi[b, i])
    return by_band
