"""CTC substitution posteriors (include/fcd.h, fcd_ctc_posterior_*) next to the two calls that walk the same lattice and
the search whose result all three read, on one GPU: BASELINE config 2 (4096 x 4000 x 5, beam 5, threshold 0.1).

    python tools/probe_posterior.py [--reps 10] [--reads 4096] [--out FILE]

Milliseconds (host clock around --inner back-to-back device-resident calls that end in one device synchronise, divided
by --inner; the median of --reps such windows after a warm-up, with the smallest and largest as *_min / *_max): the beam
search alone; ctc_score, ctc_align and ctc_posterior of hypothesis 0 of every read at band 16 and band 64, from the same
run; the bytes of forward values one posterior call writes, counted from the result's own lengths and paths (4 per live
state and row, plus an exponent word per row).  One JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def alpha_bytes(out_len, path, T, band):
    """what post_fwd_kernel stores for these labellings: 4 bytes per state of every row's live window (include/fcd.h:
    the band around the path, cut to what can be reached and can still reach the end), and 4 per row for the exponent"""
    import numpy as np
    t = np.arange(T)
    total = 0
    for L, p in zip(out_len.tolist(), path):
        k = np.searchsorted(p[:L], t, side="right")
        lo = np.maximum(np.maximum(0, 2 * (k - band) - 2), 2 * L - 2 * (T - 1 - t) - 2)
        hi = np.minimum(np.minimum(2 * L, 2 * (k + band)), 2 * t + 1)
        total += 4 * int(np.maximum(hi - lo + 1, 0).sum()) + 4 * T
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import fast_ctc_decode_amd as fcd
    from probe_align import timed
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_parity import gen_batch

    T = 4000
    x = torch.from_numpy(gen_batch(2024, args.reads, T, 5)).cuda()
    row = {"shape": "config 2", "reads": args.reads, "T": T, "reps": args.reps, "inner": args.inner}

    def put(name, fn):
        row[name + "_ms"], row[name + "_min"], row[name + "_max"] = timed(fn, args.reps, args.inner)
    put("search", lambda: fcd.beam_search_batch_raw(x, 5, 0.1))
    r = fcd.beam_search_batch_raw(x, 5, 0.1)
    rc = r.cpu()
    for band in (16, 64):
        put("score_band%d" % band, lambda: r.ctc_score(x, band=band))
        put("align_band%d" % band, lambda: r.ctc_align(x, band=band))
        put("posterior_band%d" % band, lambda: r.ctc_posterior(x, band=band))
        row["ratio_band%d" % band] = row["posterior_band%d_ms" % band] / row["score_band%d_ms" % band]
        row["alpha_bytes_band%d" % band] = alpha_bytes(rc.out_len, rc.path, T, band)
    row["mean_labels"] = float(r.out_len.float().mean())
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
