"""CTC deletion and insertion likelihoods (include/fcd.h, fcd_ctc_edits_*) next to the two calls they are measured by --
ctc_posterior, whose forward launch and backward walk they share, and ctc_score, one forward walk -- on one GPU: BASELINE
config 2 (4096 x 4000 x 5, beam 5, threshold 0.1).

    python tools/probe_edits.py [--reps 10] [--reads 4096] [--out FILE]

Milliseconds as tools/probe_posterior.py takes them (host clock around --inner back-to-back device-resident calls that end
in one device synchronise, divided by --inner; the median of --reps such windows after a warm-up, with the smallest and
largest as *_min / *_max): ctc_score, ctc_posterior and ctc_edits of hypothesis 0 of every read at band 16 and band 64,
all from the same run, and ctc_edits over ctc_posterior and over ctc_score.  One JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


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
    r = fcd.beam_search_batch_raw(x, 5, 0.1)
    for band in (16, 64):
        put("score_band%d" % band, lambda: r.ctc_score(x, band=band))
        put("posterior_band%d" % band, lambda: r.ctc_posterior(x, band=band))
        put("edits_band%d" % band, lambda: r.ctc_edits(x, band=band))
        row["edits_over_posterior_band%d" % band] = row["edits_band%d_ms" % band] / row["posterior_band%d_ms" % band]
        row["edits_over_score_band%d" % band] = row["edits_band%d_ms" % band] / row["score_band%d_ms" % band]
    row["mean_labels"] = float(r.out_len.float().mean())
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
