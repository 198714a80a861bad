"""TEST INFRASTRUCTURE shared by tests/test_ctc_edits_emu.py (the kernels on the wave64 emulator) and
tests/test_gpu_ctc_edits.py (on the GPU): the case table of tests/ctc_posterior_cases.py as it is (every
edit_back_kernel<K, NC> runs; labels enter and leave the window mid-walk; f16, bf16, time-major, ragged, both
collapse_repeats arms) and the comparison of ctc_edits_batch_raw with the float64 restatement
tests/ctc_edits_reference.py -- in exact mode every variant labelling rescored, under a band the definition on dense arrays.

Tolerance: |got - ref| <= 16 * T_r * 2^-24 + 2^-22 * |ref|.  The first term is the project's bound for a ratio of two
sums of the kind the walk accumulates (tests/ctc_posterior_cases.py: each within 6 T_r 2^-24 of its value, 16 leaves room
for the second order), which in a logarithm is an absolute error; the second is the float32 the result is stored as
(2^-24 |ref|) and its logarithm.  Where the restatement is below -100 ln 2 the contract lets the kernel drop that mass:
its value then only has to be at most -100 ln 2 plus the tolerance, -inf included.  NaN and -inf match the restatement
exactly otherwise: a variant of probability 0 is -inf, not "very small".  logp is held to ctc_score_cases.tolerance; the
condition on the inputs is ctc_score_cases.check's."""
import math

import numpy as np

import ctc_edits_reference as ER
import ctc_posterior_cases as PC
import ctc_score_cases as SC
import ctc_score_reference as R

CASES = PC.CASES
build_case = SC.build_case
FLOOR = -100.0 * math.log(2.0)
_refs = {}


def tolerance(Tr, ref):
    return 16.0 * max(Tr, 1) * 2.0 ** -24 + 2.0 ** -22 * np.abs(ref)


def reference(c, band):
    """{(b, i): (deletion (L,), insertion (L + 1, N - 1), logp)} of the case at one band; computed once, never changed"""
    key = (c["name"], band)
    if key not in _refs:
        out = {}
        B, n_hyp = c["out_len"].shape
        for b in range(B):
            Tr = c["T"] if c["lengths"] is None else int(c["lengths"][b])
            for i in range(min(n_hyp, int(c["n_valid"][b]))):
                n = int(c["out_len"][b, i])
                y, pth = c["labels"][b, i, :n], (c["paths"][b, i, :n] if band else None)
                x = c["x32"][b, :Tr]
                d, ins, lp = ER.ctc_edits(x, y, c["collapse"], band, pth)
                cond = R.ctc_logp(x, y, c["collapse"], band, pth, drop=2.0 ** -160)
                assert (lp == cond) or abs(lp - cond) <= 1e-9, ("the case relies on dropped mass", b, i, lp, cond)
                out[(b, i)] = (d, ins, lp)
        _refs[key] = out
    return _refs[key]


def check_one(got, ref, Tr, what):
    """one array of log-ratios against the restatement's; returns worst |error| / tolerance"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN where the restatement has a value, or the reverse", got, ref)
    zero = np.isneginf(ref)
    assert np.all(np.isneginf(got[zero])), (what, "a variant of probability 0 is -inf", got[zero])
    assert not np.isposinf(got).any(), what
    low = ~nan & ~zero & (ref < FLOOR)
    assert np.all(got[low] <= FLOOR + tolerance(Tr, FLOOR)), (what, "dropped mass can only lower a value", got[low], ref[low])
    rest = ~nan & ~zero & ~low
    if not rest.any():
        return 0.0
    ratio = np.abs(got[rest] - ref[rest]) / tolerance(Tr, ref[rest])
    assert ratio.max() <= 1.0, (what, "T_r", Tr, "worst |error| / tolerance", ratio.max(),
                                got[rest][ratio.argmax()], ref[rest][ratio.argmax()])
    return float(ratio.max())


def apply_edit(y, kind, pos, lab):
    y = [int(v) for v in y]
    if kind == 1:
        return tuple(y[:pos] + y[pos + 1:])
    if kind == 2:
        return tuple(y[:pos] + [lab] + y[pos:])
    if kind == 3:
        return tuple(y[:pos] + [lab] + y[pos + 1:])
    return tuple(y)


def by_variant(y, d, ins, sub=None):
    """{labelling one edit away (and y itself, 0.0): its log-ratio}.  Deleting either of two equal neighbours, or
    inserting a label on either side of an equal one, is the same labelling and -- rounding aside -- the same number:
    one edit, not two that tie."""
    out = {tuple(int(v) for v in y): 0.0}

    def put(kind, pos, lab, v):
        if v == v:
            key = apply_edit(y, kind, pos, lab)
            out[key] = max(out.get(key, -math.inf), float(v))
    for k in range(len(d)):
        put(1, k, 0, d[k])
    for g in range(ins.shape[0]):
        for c in range(ins.shape[1]):
            put(2, g, c + 1, ins[g, c])
    if sub is not None:
        for k in range(sub.shape[0]):
            for c in range(sub.shape[1]):
                if c + 1 != int(y[k]):
                    put(3, k, c + 1, sub[k, c])
    return out


def best_variant(y, d, ins, Tr, sub=None, extra=0.0):
    """-> (the best labelling, its log-ratio, decided): decided is False when the two best labellings lie within twice
    the tolerance (+ extra) of each other -- such a labelling is left out of the comparison of EditResult.best"""
    ranked = sorted(by_variant(y, d, ins, sub).items(), key=lambda kv: -kv[1])
    (v0, a), b = ranked[0], (ranked[1][1] if len(ranked) > 1 else -math.inf)
    return v0, a, bool(a - b > 2 * (tolerance(Tr, a) + extra))


def tie_share(c, band):
    """-> (labellings with a value, those of them left out of the comparison of EditResult.best)"""
    total = close = 0
    for (b, i), (d, ins, lp) in reference(c, band).items():
        if not math.isfinite(lp):
            continue
        Tr = c["T"] if c["lengths"] is None else int(c["lengths"][b])
        total += 1
        close += not best_variant(c["labels"][b, i, :d.shape[0]], d, ins, Tr)[2]
    return total, close


def check(got, c, band, verbose=True):
    """got: EditResult on numpy"""
    B, n_hyp = c["out_len"].shape
    N, stride = c["N"], c["labels"].shape[2]
    assert got.deletion.dtype == np.float32 and got.deletion.shape == (B, n_hyp, stride)
    assert got.insertion.dtype == np.float32 and got.insertion.shape == (B, n_hyp, stride + 1, N - 1)
    assert got.logp.dtype == np.float64 and got.logp.shape == (B, n_hyp)
    refs = reference(c, band)
    kind, pos, lab, val = got.best(c["out_len"])
    worst, compared, left_out = 0.0, 0, 0
    for b in range(B):
        Tr = c["T"] if c["lengths"] is None else int(c["lengths"][b])
        for i in range(n_hyp):
            if i >= int(c["n_valid"][b]):
                assert got.logp[b, i] != got.logp[b, i], ("unscored rows are NaN", b, i)
                assert kind[b, i] == 0 and val[b, i] == 0.0
                continue
            d, ins, lp = refs[(b, i)]
            assert SC.same(got.logp[b, i], lp, Tr), (c["name"], band, b, i, got.logp[b, i], lp)
            n = d.shape[0]
            what = (c["name"], "band", band, b, i)
            worst = max(worst, check_one(got.deletion[b, i, :n], d, Tr, what + ("deletion",)))
            worst = max(worst, check_one(got.insertion[b, i, :n + 1], ins, Tr, what + ("insertion",)))
            if not math.isfinite(lp):
                assert kind[b, i] == 0 and val[b, i] == 0.0, what
            else:
                want, want_val, decided = best_variant(c["labels"][b, i, :n], d, ins, Tr)
                if not decided:
                    left_out += 1
                    continue
                compared += 1
                have = apply_edit(c["labels"][b, i, :n], int(kind[b, i]), int(pos[b, i]), int(lab[b, i]))
                assert have == want, (what, "best", want, kind[b, i], pos[b, i], lab[b, i])
                assert abs(val[b, i] - want_val) <= tolerance(Tr, want_val), (what, val[b, i], want_val)
    # (which labellings are left out is decided by the restatement alone: tests/test_ctc_edits_reference.py holds their
    # share over the whole table to one in ten)
    if verbose:
        print("ctc_edits: %s band %d, %d labellings, worst |error| / tolerance = %.3f; best edit compared on %d, "
              "left out (two best within twice the tolerance) on %d" % (c["name"], band, len(refs), worst, compared, left_out))


def run_case(fcd, c, device=None):
    """the case at each of its bands (numpy through _host, or torch tensors on `device` through _dev) against the
    restatement"""
    kw = {}
    if device is None:
        xin = c["xin"]
        if c["dtype"] == "bf16":
            kw["input_dtype"] = "bfloat16"
        conv = lambda a: a
    else:
        import torch
        if c["dtype"] == "bf16":
            xin = torch.from_numpy(np.ascontiguousarray(c["xin"]).view(np.int16)).to(device).view(torch.bfloat16)
        else:
            xin = torch.from_numpy(np.ascontiguousarray(c["xin"])).to(device)
        if c["xin"].strides[0] < c["xin"].strides[1]:  # time-major on the device too
            xin = xin.transpose(0, 1).contiguous().transpose(0, 1)
        conv = lambda a: None if a is None else torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device)
    by_band = {}
    for band in c["bands"]:
        got = fcd.ctc_edits_batch_raw(xin, conv(c["labels"]), conv(c["out_len"]), c["collapse"], conv(c["lengths"]),
                                      conv(c["paths"]) if band else None, band, conv(c["n_valid"]), **kw)
        if device is not None:
            assert got.deletion.device == xin.device and got.insertion.device == xin.device and got.logp.device == xin.device
            got = got.cpu()
        check(got, c, band)
        by_band[band] = got
    return by_band


def check_edges(dele, ins, logp, x, labels, lens, lengths, unwritten):
    """dele (10, 8), ins (10, 9, 3), logp (10,) of ctc_posterior_cases.edge_batch(); entries the call must not write hold
    `unwritten`"""
    lp = logp
    assert abs(lp[0] - np.log(x[0, :, 0].astype(np.float64)).sum()) <= 6 * 2.0 ** -24 and lp[1] == 0.0
    assert lp[2] == -math.inf and lp[3] == -math.inf and lp[7] == -math.inf
    assert all(math.isnan(lp[b]) for b in (4, 5, 6, 9))
    for b in range(10):
        n = min(int(lens[b]), 8)
        if b in (0, 1, 8):  # L = 0 (gap 0 is written), L = 0 without rows (no insertion has an alignment), an ordinary row
            Tr = int(lengths[b])
            d, i, rlp = ER.ctc_edits(x[b, :Tr], labels[b, :n])
            assert SC.same(lp[b], rlp, Tr)
            check_one(dele[b, :n], d, Tr, ("edge row", b, "deletion"))
            check_one(ins[b, :n + 1], i, Tr, ("edge row", b, "insertion"))
            if b == 1:
                assert np.isneginf(ins[1, 0]).all()
            if b == 0:
                assert np.isfinite(ins[0, 0]).all()
        else:
            assert np.isnan(dele[b, :n]).all() and np.isnan(ins[b, :n + 1]).all(), (b, dele[b, :n], ins[b, :n + 1])
        assert (dele[b, n:] == unwritten).all(), (b, "entries k >= len", dele[b, n:])
        assert (ins[b, n + 1:] == unwritten).all(), (b, "entries g > len", ins[b, n + 1:])


def stray_cases():
    """NaN and +inf in cells no alignment of y = [1, 2, 3] (T = 8, N = 5) passes through, but an alignment of a shorter
    labelling does: (0, y_1) -- only y without its first label starts there -- and (T - 1, y_{L-2}) -- only y without
    its last label ends there.  -> [(x (8, 5) float32, y, bad value)]"""
    rng = np.random.default_rng(13)
    base = SC.posteriors(rng, 1, 8, 5)[0]
    out = []
    for t, col in ((0, 2), (7, 2)):
        for bad in (np.nan, np.inf):
            x = base.copy()
            x[t, col] = bad
            out.append((x, np.array([1, 2, 3], np.uint8), bad))
    return out


def check_stray(dele, ins, logp, score, x, y, bad):
    """logp is ctc_score's; a NaN shows exactly where the restatement has one; every other entry is the restatement's.
    An infinity in a cell a variant reads gives that variant "some value, nothing more" (include/fcd.h): those entries
    are not looked at, the others are held as ever."""
    d, i, lp = ER.ctc_edits(x, y)
    assert math.isfinite(lp) and SC.same(logp, lp, 8) and abs(logp - score) <= 2 * SC.tolerance(8), (logp, lp, score)
    if bad != bad:
        assert np.isnan(d).sum() == 1 and np.isnan(i).sum() == 1, (d, i)  # (the one deletion, the one insertion)
        check_one(dele, d, 8, ("stray NaN", "deletion"))
        check_one(ins, i, 8, ("stray NaN", "insertion"))
    else:
        hit_d, hit_i = ~np.isfinite(d) & ~np.isneginf(d), ~np.isfinite(i) & ~np.isneginf(i)
        assert hit_d.sum() == 1 and hit_i.sum() == 1, (d, i)
        assert np.isfinite(dele[~hit_d]).all() and not np.isnan(ins[~hit_i]).any(), (dele, ins)
        check_one(np.where(hit_d, 0.0, dele), np.where(hit_d, 0.0, d), 8, ("stray inf", "deletion"))
        check_one(np.where(hit_i, 0.0, ins), np.where(hit_i, 0.0, i), 8, ("stray inf", "insertion"))
