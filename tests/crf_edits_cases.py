"""TEST INFRASTRUCTURE shared by tests/test_crf_edits_emu.py and tests/test_crf_edits_tiers_emu.py (the kernels on the
wave64 emulator) and their GPU twins tests/test_gpu_crf_edits.py and tests/test_gpu_crf_edits_tiers.py: the shapes of
tests/crf_posterior_cases.CASES (built by crf_lattice_cases.build_case) run through crf_edits_batch_raw and compared with
the float64 restatements of tests/crf_edits_reference.py.

Every entry of every scored labelling is compared with the chain restatement (numpy, a fraction of a second per labelling),
under a band as in exact mode.  In exact mode the entries are ALSO compared with the variants rescored one by one -- a Python
loop per cell: where that would run to minutes the positions are fixed before anything runs, by the rule of
crf_posterior_cases.positions (the first and last 8 labels and gaps, the four around every multiple of 64, every 29th in
between); small cases take every position.  References are computed once per (case, band) and shared.

Tolerance, from include/fcd.h's count of roundings: |got - ref| <= 4/3 * (7 T_r 2^-24 + 2^-23 |ref|) nats -- 4/3 is the margin
the other lattice walks are tested with.  ref = -inf: -inf.  ref = NaN: NaN.  ref below -100 ln 2: the contract lets the
kernel drop cells there, the entry is a lower bound and may be -inf.  logp: crf_lattice_cases.tolerance, crf_score's."""
import math

import numpy as np

import crf_edits_reference as ER
import crf_lattice_cases as CC
import crf_lattice_reference as R
import crf_posterior_cases as PC

CASES = PC.CASES
GPU_CASES = PC.GPU_CASES
build_case = CC.build_case
DROP = -100.0 * math.log(2.0)
_refs = {}
worst_seen = {}  # (case, band) -> worst |error| / bound (the bound itself, not the tested 4/3 of it)


def bound(Tr, ref):
    return 7.0 * max(Tr, 1) * 2.0 ** -24 + 2.0 ** -23 * np.abs(ref)


def compare(got, ref_ln, logp, Tr, what):
    """got: float32 log-ratios; ref_ln: float64 ln of the variants' probabilities, same shape -> worst |error| / bound"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref_ln.shape, (what, got.shape, ref_ln.shape)
    with np.errstate(invalid="ignore"):
        ref = ref_ln - logp
    nan, ninf = np.isnan(ref), np.isneginf(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN where the restatement has a value, or the reverse", got, ref)
    assert np.isneginf(got[ninf]).all(), (what, "a variant of probability 0", got, ref)
    low = ~nan & ~ninf & (ref < DROP)
    fin = ~nan & ~ninf & ~low
    tol = 4.0 / 3.0 * bound(Tr, ref)
    assert np.all(got[low].astype(np.float64) <= ref[low] + tol[low]), (what, "below the drop threshold: a lower bound")
    if not fin.any():
        return 0.0
    err = np.abs(got[fin].astype(np.float64) - ref[fin])
    frac = float((err / bound(Tr, ref[fin])).max())
    print("crf_edits:", what, "T_r", Tr, "worst |error| / bound = %.3f" % frac)
    assert np.all(err <= tol[fin]), (what, "T_r", Tr, "worst |error| / bound", frac)
    return frac


def reference_one(x, init, y, band, pth, rescore=True):
    """-> dict(chain=(deletion, insertion, logp), pos=positions or None, rescored=(deletion[pos], insertion[gaps]) or None)"""
    y = [int(v) for v in y]
    L, N, T = len(y), x.shape[2], x.shape[0]
    d, i, lp = ER.chain(x, init, y, band, pth)
    out = dict(chain=(d, i, lp), pos=None, gaps=None, rescored=None)
    if band == 0 and rescore and math.isfinite(lp):
        pos = PC.positions(L, N, T)
        gaps = sorted(set(pos) | {L} | ({L - 1} if L else set()))
        dv, iv = ER.variants(y, N)
        rd = np.array([R.crf_score(x, init, dv[k]) for k in pos], np.float64).reshape(len(pos))
        ri = np.array([[R.crf_score(x, init, v) for v in iv[g]] for g in gaps], np.float64).reshape(len(gaps), N - 1)
        out.update(pos=pos, gaps=gaps, rescored=(rd, ri))
    return out


def reference(c, band, rescore=True):
    key = (c["name"], band, rescore)
    if key not in _refs:
        out = {}
        B, n_hyp = c["out_len"].shape
        for b in range(B):
            Tr = c["T"] if c["lengths"] is None else int(c["lengths"][b])
            for i in range(n_hyp if c["n_valid"] is None else min(n_hyp, int(c["n_valid"][b]))):
                n = int(c["out_len"][b, i])
                pth = c["paths"][b, i, :n] if band else None
                out[(b, i)] = reference_one(c["x32"][b, :Tr], c["init"][b], c["labels"][b, i, :n], band, pth, rescore)
        _refs[key] = out
    return _refs[key]


def check_one(dele, ins, ref, Tr, what):
    """one labelling's entries (deletion (L,), insertion (L + 1, N-1)) against both restatements"""
    d, i, lp = ref["chain"]
    worst = max(compare(dele, d, lp, Tr, (what, "deletion")), compare(ins, i, lp, Tr, (what, "insertion")))
    if ref["rescored"] is not None:
        rd, ri = ref["rescored"]
        worst = max(worst, compare(dele[ref["pos"]], rd, lp, Tr, (what, "deletion, rescored")),
                    compare(ins[ref["gaps"]], ri, lp, Tr, (what, "insertion, rescored")))
    return worst


def check(got, c, band, rescore=True):
    """got: EditResult on numpy"""
    B, n_hyp = c["out_len"].shape
    N, stride = c["N"], c["labels"].shape[2]
    assert got.deletion.dtype == np.float32 and got.deletion.shape == (B, n_hyp, stride)
    assert got.insertion.dtype == np.float32 and got.insertion.shape == (B, n_hyp, stride + 1, N - 1)
    assert got.logp.dtype == np.float64 and got.logp.shape == (B, n_hyp)
    refs = reference(c, band, rescore)
    worst = 0.0
    for b in range(B):
        Tr = c["T"] if c["lengths"] is None else int(c["lengths"][b])
        for i in range(n_hyp):
            n = int(c["out_len"][b, i])
            assert (got.deletion[b, i, n:] == 0).all() and (got.insertion[b, i, n + 1:] == 0).all()
            if c["n_valid"] is not None and i >= int(c["n_valid"][b]):
                assert got.logp[b, i] != got.logp[b, i], ("rows that are no hypothesis are NaN", b, i)
                assert np.isnan(got.deletion[b, i, :n]).all() and np.isnan(got.insertion[b, i, :n + 1]).all()
                continue
            lp = refs[(b, i)]["chain"][2]
            assert math.isfinite(lp), (c["name"], band, b, i, "the case is meant to have an alignment")
            assert abs(got.logp[b, i] - lp) <= CC.tolerance(Tr), (c["name"], band, b, i, got.logp[b, i], lp)
            worst = max(worst, check_one(got.deletion[b, i, :n], got.insertion[b, i, :n + 1], refs[(b, i)], Tr,
                                         (c["name"], "band", band, b, i)))
    worst_seen[(c["name"], band)] = worst
    return worst


def run_case(fcd, c, device=None, rescore=True):
    """the case at each of its bands (numpy through _host, or torch tensors on `device` through _dev)"""
    xin, conv, kw = CC._device_inputs(c, device)
    for band in c["bands"]:
        args = (xin, conv(c["init"]), conv(c["labels"]), conv(c["out_len"]), conv(c["lengths"]),
                conv(c["paths"]) if band else None, band, conv(c["n_valid"]))
        got = fcd.crf_edits_batch_raw(*args, **kw)
        score = fcd.crf_score_batch_raw(*args, **kw)
        if device is not None:
            assert got.deletion.device == xin.device and got.insertion.device == xin.device and got.logp.device == xin.device
            score = score.cpu().numpy()
        got = got.cpu()
        ok = np.isfinite(score)
        assert np.array_equal(np.isnan(got.logp), np.isnan(score)) and np.array_equal(np.isfinite(got.logp), ok)
        # (the same value, or the last bits of the float64 logarithm: the forward pass keeps one more state a row)
        assert np.all(np.abs(got.logp[ok] - score[ok]) <= 2.0 ** -40 * np.maximum(1.0, np.abs(score[ok]))), (c["name"], band)
        check(got, c, band, rescore)


# ---- cases outside the table, shared by the emulator files and their GPU twins (device=None: numpy through _host) ----
_conv = PC._conv


def edits(fcd, device, x, init, labels, lens, lengths=None, paths=None, band=0):
    to = _conv(device)
    return fcd.crf_edits_batch_raw(to(x), to(init), to(labels), to(lens), to(lengths), to(paths) if band else None, band).cpu()


def edge_rows(fcd, device=None):
    """crf_posterior_cases.edge_batch: the rows without a value, T_r = L (row 7), an ordinary row (8), and row 10 -- a NaN
    that only variants read: NaN in their entries alone, logp as it is"""
    x, init, labels, lens, lengths = PC.edge_batch()
    got = edits(fcd, device, x, init, labels, lens, lengths)
    lp = got.logp[:, 0]
    assert lp[1] == 0.0 and lp[2] == -math.inf and lp[3] == -math.inf and lp[11] == -math.inf
    assert all(math.isnan(lp[b]) for b in (4, 5, 6, 9))
    for b in range(12):
        n = min(int(lens[b]), 8)
        Tr = int(lengths[b])
        dele, ins = got.deletion[b, 0], got.insertion[b, 0]
        assert (dele[n:] == 0).all() and (ins[n + 1:] == 0).all(), (b, "entries beyond the labelling")
        if b in (0, 7, 8, 10):
            ref = reference_one(x[b, :Tr], init[b], labels[b, :n], 0, None, rescore=b != 10)
            assert math.isfinite(ref["chain"][2]) and abs(lp[b] - ref["chain"][2]) <= CC.tolerance(6), b
            check_one(dele[:n], ins[:n + 1], ref, 6, "edge row %d" % b)
        elif b == 1:  # T_r = 0, L = 0: P(y | x) = 1, no insertion has an alignment
            assert np.isneginf(ins[0]).all()
        else:
            assert np.isnan(dele[:n]).all() and np.isnan(ins[:n + 1]).all(), (b, dele, ins)
    assert np.isneginf(got.insertion[7, 0, :7]).all() and np.isfinite(got.deletion[7, 0, :6]).all()  # T_r = L
    assert got.deletion[0, 0].tolist() == [0.0] * 8 and np.isfinite(got.insertion[0, 0, 0]).all()      # L = 0: gap 0 alone
    d10, i10 = got.deletion[10, 0, :2], got.insertion[10, 0, :3]
    assert math.isfinite(lp[10]) and np.isnan(i10).any() and np.isfinite(i10).any() and not np.isnan(d10).all()
    # the rescored variants agree on which entries the NaN reaches wherever both have a value or both have none
    rd, ri, _ = ER.rescored(x[10], init[10], labels[10, :2])
    assert np.isnan(i10)[np.isnan(ri)].all() and np.isnan(d10)[np.isnan(rd)].all()
    return got


def heavy_variants(fcd, device=None):
    """edits that outweigh the called labelling by more than f32 has exponent (crf_posterior_cases.heavy_variants' reads): the
    accumulators' own exponent holds them"""
    rng = np.random.default_rng(80)
    x = CC.posteriors(rng, 2, 8, 4, 5)
    init = np.array([[0.9, 0.1, 0.2, 0.3], [0.1, 0.2, 0.9, 0.3]], np.float32)  # sigma_0 = 0, 2
    labels = np.zeros((2, 8), np.uint8)
    labels[0, :3], labels[1, :1] = [2, 3, 1], [1]
    lens = np.array([3, 1], np.uint32)
    lengths = np.array([8, 4], np.int64)
    x[0, :, 1, 3] = 1e-30
    x[0, :, 2, :] *= np.float32(1e-12)
    x[1, :, 2, 0], x[1, :, 2, 1] = 1e-20, 2e-38
    x[1, 3, 2, 1:] = 0.0
    x[1, :, 0, :] *= np.float32(1e-6)
    got = edits(fcd, device, x, init, labels, lens, lengths)
    heavy = 0
    for b in range(2):
        n, Tr = int(lens[b]), int(lengths[b])
        ref = reference_one(x[b, :Tr], init[b], labels[b, :n], 0, None)
        d, i, lp = ref["chain"]
        assert math.isfinite(lp) and abs(got.logp[b, 0] - lp) <= CC.tolerance(Tr)
        heavy += int(max(d.max(), i.max()) - lp > 130 * math.log(2.0))
        check_one(got.deletion[b, 0, :n], got.insertion[b, 0, :n + 1], ref, Tr, ("heavy variants", b))
    assert heavy == 2, "the case is meant to be lopsided"


def best_edit_is_crf_score(fcd, device=None):
    """crf_edits of a crf_beam_search result next to its crf_posterior: EditResult.best's pick, applied to the labelling and
    scored by crf_score, has the log-ratio best() reports"""
    rng = np.random.default_rng(31)
    to = _conv(device)
    x = CC.posteriors(rng, 6, 48, 16, 5, sharp=0.3)
    init = rng.random((6, 16)).astype(np.float32)
    lengths = np.array([48, 30, 48, 7, 41, 48], np.int64)
    r = fcd.crf_beam_search_batch_raw(to(x), to(init), 2, 0.0, lengths=to(lengths))  # (a narrow beam: edits that help exist)
    ed = r.crf_edits(to(x), to(init), lengths=to(lengths))
    po = r.crf_posterior(to(x), to(init), lengths=to(lengths))
    rc = r.cpu()
    kind, pos, lab, ratio = ed.best(rc.out_len, po, rc.labels)
    e = ed.cpu()
    assert e.deletion.shape == (6, 1, 48) and e.insertion.shape == (6, 1, 49, 4)
    assert np.allclose(e.logp, po.cpu().logp, rtol=0, atol=CC.tolerance(48))
    kinds = set()
    for b in range(6):
        n, Tr = int(rc.out_len[b]), int(lengths[b])
        y = [int(v) for v in rc.labels[b, :n]]
        k, p, c = int(kind[b, 0]), int(pos[b, 0]), int(lab[b, 0])
        kinds.add(k)
        if k == 0:
            continue
        v = y[:p] + y[p + 1:] if k == 1 else (y[:p] + [c] + y[p:] if k == 2 else y[:p] + [c] + y[p + 1:])
        want = R.crf_score(x[b, :Tr], init[b], v) - R.crf_score(x[b, :Tr], init[b], y)
        assert ratio[b, 0] > 0 and abs(ratio[b, 0] - want) <= 4.0 / 3.0 * (2 * bound(Tr, want) + 16 * 2.0 ** -24), (b, k, p, c, ratio[b, 0], want)
    assert kinds - {0}, "the case is meant to hold a labelling that an edit improves"
    return kinds


def argument_errors(fcd):
    """the C ABI refuses bad calls itself, before anything is enqueued or written (host layer; numpy)"""
    import ctypes as C

    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(6)
    x = CC.posteriors(rng, 2, 10, 4, 5)
    init = np.ones((2, 4), np.float32)
    labels = np.ones((2, 10), np.uint8)
    lens = np.array([3, 4], np.uint32)
    h = nat.default_handle()
    path = np.zeros((2, 10), np.uint32)
    de, ins, lp = np.full((2, 10), 77.0, np.float32), np.full((2, 11, 4), 77.0, np.float32), np.full(2, 77.0)

    def call(fn, S=4, n_hyp=1, band=0, with_path=True, dele=True, insr=True, logp=True, with_init=True, n_init=4, out=True):
        b = nat.Batch(x.ctypes.data, 2, 10, S, 5, 200, 20, 5, 1, None)
        y = nat.Labellings(labels.ctypes.data, lens.ctypes.data, None, path.ctypes.data if with_path else None, n_hyp, 10)
        o = nat.Edits(de.ctypes.data if dele else None, ins.ctypes.data if insr else None, lp.ctypes.data if logp else None)
        return getattr(h.lib, fn)(h.ptr, C.byref(b), init.ctypes.data if with_init else None, n_init, 4, C.byref(y), band,
                                  C.byref(o) if out else None)
    for fn in ("fcd_crf_edits_host", "fcd_crf_edits_dev"):
        assert call(fn, band=-1) == nat.E_INVALID
        assert call(fn, band=3, with_path=False) == nat.E_INVALID
        assert call(fn, n_hyp=0) == nat.E_INVALID
        assert call(fn, S=0) == nat.E_INVALID
        assert call(fn, with_init=False) == nat.E_INVALID
        assert call(fn, n_init=0) == nat.E_INVALID
        assert call(fn, out=False) == nat.E_INVALID
        assert call(fn, dele=False) == nat.E_INVALID
        assert call(fn, insr=False) == nat.E_INVALID
    assert (de == 77).all() and (ins == 77).all() and (lp == 77).all()
    assert call("fcd_crf_edits_host", logp=False) == nat.OK and (lp == 77).all() and np.isfinite(de[0, :3]).all()
    assert call("fcd_crf_edits_host") == nat.OK and np.isfinite(lp).all()
    # the limits are crf_posterior's, and the message names crf_edits and the way out
    for T, S, N, band, msg in ((40, 5, 4, 0, b"power of N - 1"), (40, 9, 10, 0, b"8 labels"), (512, 4, 5, 0, b"use a band"),
                               (192, 64, 5, 0, b"band of at most 95"), (600, 1024, 5, 96, b"band of at most 95"),
                               (600, 8, 9, 128, b"band of at most 127"),
                               (40, 16384, 5, 4, b"more labels than the kernels carry")):
        b = nat.Batch(None, 0, T, S, N, T * S * N, S * N, N, 1, None)
        y = nat.Labellings(None, None, None, path.ctypes.data, 1, T)
        assert h.lib.fcd_crf_edits_host(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(y), band,
                                        C.byref(nat.Edits(None, None, None))) == nat.E_UNSUPPORTED
        err = h.lib.fcd_last_error(h.ptr)
        assert msg in err and (b"crf_edits" in err or b"crf lattice" in err), err
    for T, S, N, band in ((511, 4, 5, 0), (600, 16, 5, 255), (191, 64, 5, 0), (600, 4096, 5, 95), (600, 8, 3, 255),
                          (600, 8, 9, 127), (255, 1, 9, 0)):
        b = nat.Batch(None, 0, T, S, N, T * S * N, S * N, N, 1, None)
        y = nat.Labellings(None, None, None, path.ctypes.data, 1, T)
        assert h.lib.fcd_crf_edits_host(h.ptr, C.byref(b), init.ctypes.data, 4, 4, C.byref(y), band,
                                        C.byref(nat.Edits(None, None, None))) == nat.OK, (T, S, N, band)


def workspace_limit_groups(fcd, device=None):
    """a workspace limit of one byte: every read is a launch trio of its own, in the same memory; the same values"""
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(8)
    to = _conv(device)
    x = CC.posteriors(rng, 6, 40, 16, 5)
    init = rng.random((6, 16)).astype(np.float32)
    lengths = np.array([40, 17, 40, 1, 33, 40], np.int64)
    h = nat.default_handle() if device is None else nat.default_handle(0)
    r = fcd.crf_beam_search_batch_raw(to(x), to(init), 5, 0.0, lengths=to(lengths))
    for band in (0, 4):
        whole = r.crf_edits(to(x), to(init), lengths=to(lengths), band=band).cpu()
        h.set_workspace_limit(1)
        try:
            parts = r.crf_edits(to(x), to(init), lengths=to(lengths), band=band).cpu()
        finally:
            h.set_workspace_limit(0)
        assert np.array_equal(whole.deletion, parts.deletion, equal_nan=True)
        assert np.array_equal(whole.insertion, parts.insertion, equal_nan=True) and np.array_equal(whole.logp, parts.logp)
        assert np.isfinite(whole.logp[:, 0]).all()


# ---- one small call per instantiation the edits run on ----
TIER_SHAPES = {(1, 8): (8, 9), (2, 4): (16, 5), (4, 2): (8, 3), (3, 8): (64, 5), (6, 4): (1024, 5)}  # (MM, NB) -> (S, N)
TIER_ROWS = {1: 40, 2: 64, 3: 128, 4: 128, 8: 256}  # K -> T; stride = T, exact mode: a window of T + 1 states
TIERS = [(k, mm, nb) for mm, nb in ((2, 4), (4, 2)) for k in (1, 2, 4, 8)] + [(k, 1, 8) for k in (1, 2, 4)] + \
        [(k, mm, nb) for mm, nb in ((3, 8), (6, 4)) for k in (1, 2, 3)]  # every one carries the edit walks


def tier_call(fcd, tier, device=None):
    """-> (EditResult on numpy, x, init, labels, lens) of one read of the tier's shape; checked against the chain restatement,
    and at the positions of crf_posterior_cases.positions against the rescored variants"""
    k, mm, nb = tier
    S, N = TIER_SHAPES[(mm, nb)]
    T = TIER_ROWS[k]
    rng = np.random.default_rng(900 + 100 * k + 10 * mm + nb)
    x = CC.posteriors(rng, 1, T, S, N)
    init = rng.random((1, S)).astype(np.float32)
    L = int(0.7 * T)
    labels = np.zeros((1, T), np.uint8)
    labels[0, :L] = rng.integers(1, N, L)
    lens = np.array([L], np.uint32)
    got = edits(fcd, device, x, init, labels, lens)
    return got, x, init, labels, lens


def tier_check(got, x, init, labels, lens, tier):
    L, T = int(lens[0]), x.shape[1]
    d, i, lp = ER.chain(x[0], init[0], labels[0, :L])
    assert math.isfinite(lp) and abs(got.logp[0, 0] - lp) <= CC.tolerance(T)
    ref = dict(chain=(d, i, lp), pos=None, gaps=None, rescored=None)
    pos = [0, 1, L // 2, L - 2, L - 1]  # (and a few positions rescored: the definition itself)
    dv, iv = ER.variants(labels[0, :L], x.shape[3])
    ref.update(pos=pos, gaps=pos + [L],
               rescored=(np.array([R.crf_score(x[0], init[0], dv[k]) for k in pos]),
                         np.array([[R.crf_score(x[0], init[0], v) for v in iv[g]] for g in pos + [L]])))
    return check_one(got.deletion[0, 0, :L], got.insertion[0, 0, :L + 1], ref, T, ("tier", tier))
