"""CRF motif spotting (include/fcd.h, fcd_crf_spot_*) next to crf_detect on the same inputs and next to the alignment call
whose kernels it shares, on one GPU.

    python tools/probe_crf_spot.py [--states 4] [--reads 4096] [--T 400] [--rows 400] [--labels 24] [--reps 10] [--inner 40] [--out FILE]

tools/probe_crf_detect.py's protocol and inputs (milliseconds: host clock around --inner back-to-back device-resident calls
that end in one device synchronise, divided by --inner; the median of --reps such windows after a warm-up, with the smallest
and largest as *_min / *_max).  crf_align: 120 random labels a read at bands 16 and 64 around an evenly spread path (the
shared kernels with spotting off), and crf_detect at 24 motifs: both run on a library without crf_spot_batch_raw -- an older
commit -- too, which reports them alone.  crf_spot: 4, 24 and 96 motifs of --labels labels in the first --rows rows, without
spans, and with spans and the track.  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=4)
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--T", type=int, default=400)
    ap.add_argument("--rows", type=int, default=400)
    ap.add_argument("--labels", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import fast_ctc_decode_amd as fcd
    from probe_align import timed

    B, T, S, N = args.reads, args.T, args.states, 5
    g = torch.Generator(device="cuda").manual_seed(2024)
    scores = torch.randn((B, T, S, N), generator=g, device="cuda")
    tr = fcd.crf_transition_probs_batch_raw(scores)
    marg = fcd.crf_marginals_batch_raw(scores, emit=False).marginals
    row = {"states": S, "reads": B, "T": T, "rows": args.rows, "labels": args.labels, "reps": args.reps, "inner": args.inner}

    def put(name, fn):
        row[name + "_ms"], row[name + "_min"], row[name + "_max"] = timed(fn, args.reps, args.inner)
    rng = np.random.default_rng(7)
    lab = torch.from_numpy(rng.integers(1, N, size=(B, 120)).astype(np.uint8)).cuda()
    n = torch.full((B,), 120, dtype=torch.int32, device="cuda")
    paths = torch.from_numpy(np.tile((np.arange(120) * T // 120).astype(np.uint32).view(np.int32), (B, 1))).cuda()
    for band in (16, 64):
        put("crf_align_band%d" % band, lambda: fcd.crf_align_batch_raw(tr.probs, tr.init, lab, n, paths=paths, band=band))
    sets = {M: rng.integers(1, N, size=(M, args.labels)).astype(np.uint8) for M in (4, 24, 96)}
    lens = np.full(24, args.labels, np.uint32)  # (the shared path first: at the same place in an older commit's run)
    put("crf_detect_M24", lambda: fcd.crf_detect_batch_raw(tr.probs, marg, sets[24], lens, rows=(0, args.rows)))
    for M, motifs in sets.items():
        lens = np.full(M, args.labels, np.uint32)
        if hasattr(fcd, "crf_spot_batch_raw"):
            if M != 24:
                put("crf_detect_M%d" % M, lambda: fcd.crf_detect_batch_raw(tr.probs, marg, motifs, lens, rows=(0, args.rows)))
            put("crf_spot_M%d" % M, lambda: fcd.crf_spot_batch_raw(tr.probs, marg, motifs, lens, rows=(0, args.rows)))
            put("crf_spot_M%d_spans_track" % M,
                lambda: fcd.crf_spot_batch_raw(tr.probs, marg, motifs, lens, rows=(0, args.rows), track=True, spans=True))
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
