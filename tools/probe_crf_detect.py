"""CRF motif occurrence posteriors (include/fcd.h, fcd_crf_detect_*) next to the scoring call whose kernels they share, and
next to ctc_detect on plain-CTC posteriors of the same batch size as a plausibility figure, on one GPU.

    python tools/probe_crf_detect.py [--states 4] [--reads 4096] [--T 400] [--rows 400] [--labels 24] [--reps 10] [--inner 40] [--out FILE]

tools/probe_detect.py's protocol (milliseconds: host clock around --inner back-to-back device-resident calls that end in one
device synchronise, divided by --inner; the median of --reps such windows after a warm-up, with the smallest and largest as
*_min / *_max).  Seeded N(0, 1) scores (reads, T, states, 5) go through crf_transition_probs_batch_raw and
crf_marginals_batch_raw once, outside the clock.  crf_score: 120 random labels a read (the shared path: the same kernels with
detecting off; a library without crf_detect_batch_raw -- an older commit -- reports this alone).  crf_detect: 4, 24 and 96
motifs of --labels labels in the first --rows rows, without and (4 motifs) with the track; ctc_detect unpacked at the same
reads, motifs and rows.  One JSON line."""
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
    row = {"states": S, "reads": B, "T": T, "rows": args.rows, "labels": args.labels, "reps": args.reps, "inner": args.inner}

    def put(name, fn):
        row[name + "_ms"], row[name + "_min"], row[name + "_max"] = timed(fn, args.reps, args.inner)
    rng = np.random.default_rng(7)
    lab = torch.from_numpy(rng.integers(1, N, size=(B, 120)).astype(np.uint8)).cuda()
    n = torch.full((B,), 120, dtype=torch.int32, device="cuda")
    put("crf_score", lambda: fcd.crf_score_batch_raw(tr.probs, tr.init, lab, n))
    if hasattr(fcd, "crf_detect_batch_raw"):
        marg = fcd.crf_marginals_batch_raw(scores, emit=False).marginals
        ctc = torch.softmax(scores[:, :, 0, :], dim=-1).contiguous()
        for M in (4, 24, 96):
            motifs = rng.integers(1, N, size=(M, args.labels)).astype(np.uint8)
            lens = np.full(M, args.labels, np.uint32)
            put("crf_detect_M%d" % M, lambda: fcd.crf_detect_batch_raw(tr.probs, marg, motifs, lens, rows=(0, args.rows)))
            if M == 4:
                put("crf_detect_M4_track", lambda: fcd.crf_detect_batch_raw(tr.probs, marg, motifs, lens, rows=(0, args.rows), track=True))
            put("ctc_detect_M%d" % M, lambda: fcd.ctc_detect_batch_raw(ctc, motifs, lens, rows=(0, args.rows)))
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
