"""CRF deletion and insertion likelihoods (include/fcd.h, fcd_crf_edits_*) next to crf_posterior -- one forward and one
backward walk of the same kernels -- and crf_score, which walks the same lattice forward only, on one GPU.

    python tools/probe_crf_edits.py [--reps 5] [--reads 4096] [--large-reads 256] [--out FILE]

BASELINE config 4's shape (4096 x 4000 x 4 states x 5, beam 5): crf_score, crf_posterior and crf_edits of every read's result
at band 16 and band 64, from the same run, the ratio of crf_edits to each, and the number of crf_score calls that rescoring
every variant would take (L + (L + 1)(N - 1) at the mean L).  One S = 1024 case (f16, gathered rows, a history of five labels) at band 16.  Milliseconds as
tools/probe_posterior.py takes them: the host clock around --inner back-to-back device-resident calls that end in one device
synchronise, divided by --inner; the median of --reps such windows after a warm-up, with the smallest and largest as
*_min / *_max.  One JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--large-reads", type=int, default=256)
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import fast_ctc_decode_amd as fcd
    from probe_align import timed
    from probe_crf_lattice import crf_batch

    T = args.rows
    row = {"shape": "config 4", "reads": args.reads, "T": T, "reps": args.reps, "inner": args.inner}

    def put(name, fn):
        row[name + "_ms"], row[name + "_min"], row[name + "_max"] = timed(fn, args.reps, args.inner)
    x = crf_batch(torch, 4, args.reads, T, 4, 5, torch.float32)
    init = torch.rand((args.reads, 4), device="cuda")
    r = fcd.crf_beam_search_batch_raw(x, init, 5, 0.0)
    row["mean_labels"] = float(r.out_len.float().mean())
    row["rescoring_calls"] = row["mean_labels"] + (row["mean_labels"] + 1) * 4
    for band in (16, 64):
        put("score_band%d" % band, lambda: r.crf_score(x, init, band=band))
        put("posterior_band%d" % band, lambda: r.crf_posterior(x, init, band=band))
        put("edits_band%d" % band, lambda: r.crf_edits(x, init, band=band))
        row["edits_over_posterior_band%d" % band] = row["edits_band%d_ms" % band] / row["posterior_band%d_ms" % band]
        row["edits_over_score_band%d" % band] = row["edits_band%d_ms" % band] / row["score_band%d_ms" % band]
    del x, r
    n = args.large_reads
    if n > 0:
        xl = crf_batch(torch, 5, n, T, 1024, 5, torch.float16)
        il = torch.rand((n, 1024), device="cuda")
        rl = fcd.crf_beam_search_batch_raw(xl, il, 5, 0.0)
        row["large_reads"], row["large_S"] = n, 1024
        row["large_mean_labels"] = float(rl.out_len.float().mean())
        put("large_score_band16", lambda: rl.crf_score(xl, il, band=16))
        put("large_posterior_band16", lambda: rl.crf_posterior(xl, il, band=16))
        put("large_edits_band16", lambda: rl.crf_edits(xl, il, band=16))
        row["large_edits_over_posterior_band16"] = row["large_edits_band16_ms"] / row["large_posterior_band16_ms"]
        row["large_edits_over_score_band16"] = row["large_edits_band16_ms"] / row["large_score_band16_ms"]
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
