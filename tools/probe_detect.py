"""CTC motif occurrence posteriors (include/fcd.h, fcd_ctc_detect_*) next to motif spotting and the scoring call whose
kernels they share, on one GPU: BASELINE config 2's batch (4096 x 4000 x 5, beam 5, threshold 0.1).

    python tools/probe_detect.py [--reps 20] [--inner 10] [--reads 4096] [--motifs 4] [--labels 24] [--rows 400] [--packed] [--out FILE]

tools/probe_spot.py's protocol (milliseconds: host clock around --inner back-to-back device-resident calls that end in
one device synchronise, divided by --inner; the median of --reps such windows after a warm-up, with the smallest and
largest as *_min / *_max): ctc_score of every read's search result at band 16 and band 64 (the shared path: the same
kernels with detecting off); --motifs motifs of --labels labels in the first --rows rows of every read through
ctc_detect_batch_raw and ctc_spot_batch_raw, without and with the track.  A library without ctc_detect_batch_raw (an
older commit) reports the rest.  --packed adds ctc_detect_batch_raw(packed=True) -- one (read, motif) pair per lane
 -- at the same shape, and whether its end rows equal the unpacked call's.  One JSON line."""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--motifs", type=int, default=4)
    ap.add_argument("--labels", type=int, default=24)
    ap.add_argument("--rows", type=int, default=400)
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import fast_ctc_decode_amd as fcd
    from probe_align import timed
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_parity import gen_batch

    T = 4000
    x = torch.from_numpy(gen_batch(2024, args.reads, T, 5)).cuda()
    row = {"shape": "config 2", "reads": args.reads, "T": T, "reps": args.reps, "inner": args.inner,
           "motifs": args.motifs, "labels": args.labels, "rows": args.rows}

    def put(name, fn):
        row[name + "_ms"], row[name + "_min"], row[name + "_max"] = timed(fn, args.reps, args.inner)
    r = fcd.beam_search_batch_raw(x, 5, 0.1)
    for band in (16, 64):
        put("score_band%d" % band, lambda: r.ctc_score(x, band=band))
    rng = np.random.default_rng(7)
    motifs = rng.integers(1, 5, size=(args.motifs, args.labels)).astype(np.uint8)
    lens = np.full(args.motifs, args.labels, np.uint32)
    for kind in ("spot", "detect"):
        call = getattr(fcd, "ctc_%s_batch_raw" % kind, None)
        if call is not None:
            for name, track in ((kind, False), (kind + "_track", True)):
                put(name, lambda: call(x, motifs, lens, rows=(0, args.rows), track=track))
    if args.packed:
        put("detect_packed", lambda: fcd.ctc_detect_batch_raw(x, motifs, lens, rows=(0, args.rows), packed=True))
        a = fcd.ctc_detect_batch_raw(x, motifs, lens, rows=(0, args.rows), packed=True).cpu()
        b = fcd.ctc_detect_batch_raw(x, motifs, lens, rows=(0, args.rows)).cpu()
        row["packed_end_equal"] = bool(np.array_equal(a.end, b.end))
        row["packed_count_bits_equal"] = bool(np.array_equal(a.count, b.count, equal_nan=True))
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
