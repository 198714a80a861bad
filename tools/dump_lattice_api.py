#!/usr/bin/env python3
"""Dump everything the ten labelling-lattice calls of the Python layer return, for comparing two commits whose compiled
code is the same: run it at both, then `--compare A.npz B.npz` -- every array must be equal, dtype and shape included.

    python tools/dump_lattice_api.py --emu OUT.npz       numpy in, on the CPU emulation of the kernels (no GPU)
    python tools/dump_lattice_api.py --device OUT.npz    torch device tensors in, float32 and float16 posteriors
    python tools/dump_lattice_api.py --compare A.npz B.npz

The inputs are fixed: 3 ragged reads (12, 7 and 0 rows of 12), N = 5, S = 4 for the CRF calls, 2 labellings per read of
which n_valid = [2, 1, 0] count, one empty labelling and one longer than its read; band 0, and band 2 with paths.  The two
occupancy calls also run with out= (full rank, and the reduced rank of one labelling per read), accumulate=True with
scale=-1, time_major_out=True and wide=True.  The result methods of a plain, an n-best and a CRF search and the ten
single-read functions are dumped with them.  A key is "<call>|<variant>|<field>|<container type>|<dtype>"; next to every
array its strides are kept under "...|strides"."""
import argparse
import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("score", "align", "posterior", "edits", "occupancy")
FIELDS = {"AlignResult": ("start", "count", "qual", "logp"), "PosteriorResult": ("post", "logp"),
          "EditResult": ("deletion", "insertion", "logp"), "OccupancyResult": ("occupancy", "logp")}
B, T, N, S, H, STRIDE = 3, 12, 5, 4, 2, 9
LENGTHS = [12, 7, 0]
N_VALID = [2, 1, 0]
LABEL_LENGTHS = [[5, 0], [9, 4], [0, 0]]  # (read 0, 1): empty; (read 1, 0): 9 labels for 7 rows


def inputs():
    rng = np.random.default_rng(20240607)
    x = rng.random((B, T, N)).astype(np.float32) + 0.05
    x /= x.sum(-1, keepdims=True)
    xc = rng.random((B, T, S, N)).astype(np.float32) + 0.05
    xc /= xc.sum((-2, -1), keepdims=True)
    init = rng.random((B, S)).astype(np.float32)
    labels = rng.integers(1, N, (B, H, STRIDE)).astype(np.uint8)
    paths = np.zeros((B, H, STRIDE), np.uint32)
    for b in range(B):
        for i in range(H):
            rows = np.sort(rng.integers(0, max(LENGTHS[b], 1), LABEL_LENGTHS[b][i]))
            paths[b, i, :len(rows)] = rows
    return dict(x=x, xc=xc, init=init, labels=labels, paths=paths, ylen=np.array(LABEL_LENGTHS, np.uint32),
                lengths=np.array(LENGTHS, np.int64), n_valid=np.array(N_VALID, np.uint32))


class Dump:
    def __init__(self):
        self.arrays = {}

    def add(self, call, variant, field, a):
        kind = "%s.%s" % (type(a).__module__.split(".")[0], type(a).__name__)
        if isinstance(a, np.ndarray):
            host, strides = a, a.strides
        elif isinstance(a, (float, int, str, list, tuple)):
            host, strides = np.asarray(a), ()
        else:
            host, strides = a.cpu().numpy(), tuple(a.stride())
        key = "|".join((call, variant, field, kind, str(getattr(a, "dtype", type(a).__name__))))
        assert key not in self.arrays, key
        self.arrays[key] = host
        self.arrays[key + "|strides"] = np.asarray(strides, np.int64)

    def result(self, call, variant, r):
        fields = FIELDS.get(type(r).__name__)
        if fields is None:
            self.add(call, variant, "logp", r)
        else:
            for f in fields:
                self.add(call, variant, f, getattr(r, f))


def dump_batch_calls(fcd, d, conv, tag, half):
    """the ten *_batch_raw calls; conv puts a numpy array where the inputs live"""
    v = inputs()
    f16 = (lambda a: a.astype(np.float16)) if half else (lambda a: a)
    lab, ylen, pth = conv(v["labels"]), conv(v["ylen"]), conv(v["paths"])
    lengths, n_valid = conv(v["lengths"]), conv(v["n_valid"])
    for model in ("ctc", "crf"):
        x = conv(f16(v["xc" if model == "crf" else "x"]))
        head = (x, conv(v["init"])) if model == "crf" else (x,)
        cell = (T, S, N) if model == "crf" else (T, N)
        for kind in KINDS:
            call = "%s_%s_batch_raw" % (model, kind)
            f = getattr(fcd, call)
            for band in (0, 2):
                kw = dict(lengths=lengths, n_valid=n_valid, band=band, paths=pth if band else None)
                d.result(call, "%s.band%d" % (tag, band), f(*head, lab, ylen, **kw))
                if kind != "occupancy":
                    continue
                name = "%s.band%d." % (tag, band)
                out = conv(np.full((B, H) + cell, 0.25, np.float32))
                r = f(*head, lab, ylen, out=out, **kw)
                assert r.occupancy is out
                d.result(call, name + "out", r)
                d.result(call, name + "accumulate", f(*head, lab, ylen, out=out, accumulate=True, scale=-1.0, **kw))
                one = conv(np.full((B,) + cell, 0.5, np.float32))
                kw1 = dict(lengths=lengths, band=band, paths=pth[:, 0] if band else None)
                d.result(call, name + "out_reduced", f(*head, lab[:, 0], ylen[:, 0], out=one, **kw1))
                d.result(call, name + "time_major", f(*head, lab, ylen, time_major_out=True, **kw))
                d.result(call, name + "wide", f(*head, lab, ylen, wide=True, **kw))
            if model == "ctc":
                d.result(call, tag + ".no_collapse", f(*head, lab, ylen, False, lengths=lengths, n_valid=n_valid))
        if model == "crf":
            d.result("crf_score_batch_raw", tag + ".wide", fcd.crf_score_batch_raw(*head, lab, ylen, lengths=lengths,
                                                                                   n_valid=n_valid, wide=True))


def dump_result_methods(fcd, d, conv, tag):
    """the ten methods of the searches' results, on the arrays the searches returned"""
    v = inputs()
    x, xc, init, lengths = conv(v["x"]), conv(v["xc"]), conv(v["init"]), conv(v["lengths"])
    plain = {"batch": fcd.beam_search_batch_raw(x, 5, 0.0, lengths=lengths),
             "nbest": fcd.beam_search_nbest_batch_raw(x, 2, 5, 0.0, lengths=lengths)}
    crf = {"batch": fcd.crf_beam_search_batch_raw(xc, init, 5, 0.0, lengths=lengths),
           "nbest": fcd.crf_beam_search_nbest_batch_raw(xc, init, 2, 5, 0.0, lengths=lengths)}
    for kind in KINDS:
        for band in (0, 2):
            for name, r in plain.items():
                d.result("%s.ctc_%s" % (name, kind), "%s.band%d" % (tag, band),
                         getattr(r, "ctc_" + kind)(x, lengths=lengths, band=band))
            for name, r in crf.items():
                d.result("%s.crf_%s" % (name, kind), "%s.band%d" % (tag, band),
                         getattr(r, "crf_" + kind)(xc, init, lengths=lengths, band=band))


def dump_single_reads(fcd, d, tag):
    v = inputs()
    x, xc, init = v["x"][1, :7], v["xc"][1, :7], v["init"][1]
    for seq in ("", "ACGTA", "ACCA"):
        for kind in KINDS:
            for call, got in (("ctc_" + kind, getattr(fcd, "ctc_" + kind)(x, seq, "NACGT")),
                              ("crf_" + kind, getattr(fcd, "crf_" + kind)(xc, init, seq, "NACGT"))):
                for i, part in enumerate(got if isinstance(got, tuple) else (got,)):
                    d.add(call, "%s.%s" % (tag, seq or "empty"), "part%d" % i, part)


def run(mode):
    sys.path.insert(0, ROOT)
    d = Dump()
    if mode == "emu":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from emu_util import emulated_kernels
        ctx = emulated_kernels()
    else:
        ctx = contextlib.nullcontext()
    import fast_ctc_decode_amd as fcd
    with ctx:
        if mode == "emu":
            dump_batch_calls(fcd, d, lambda a: a, "numpy", False)
            dump_result_methods(fcd, d, lambda a: a, "numpy")
        else:
            import torch

            def conv(a):
                if a.dtype == np.uint32:
                    a = a.view(np.int32)  # (the searches' device results are int32 tensors)
                return torch.from_numpy(a).cuda()
            dump_batch_calls(fcd, d, conv, "f32", False)
            dump_batch_calls(fcd, d, conv, "f16", True)
            dump_result_methods(fcd, d, conv, "f32")
            torch.cuda.synchronize()
        dump_single_reads(fcd, d, "numpy")
    return d.arrays


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        u, w = a[k], b[k]
        same = u.dtype == w.dtype and u.shape == w.shape and (
            np.array_equal(u, w, equal_nan=True) if u.dtype.kind in "fc" else np.array_equal(u, w))
        if not same:
            bad.append(k)
    for k in bad:
        print("DIFFERS", k)
    print("%d arrays in %s, %d in %s, %d differ" % (len(a.files), path_a, len(b.files), path_b, len(bad)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--emu", metavar="OUT", help="numpy inputs on the CPU emulation of the kernels")
    g.add_argument("--device", metavar="OUT", help="torch device tensors on the GPU")
    g.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    arrays = run("emu" if a.emu else "device")
    np.savez(a.emu or a.device, **arrays)
    print("%d arrays -> %s" % (len(arrays), a.emu or a.device))
    return 0


if __name__ == "__main__":
    sys.exit(main())
