"""CTC forward scoring (include/fcd.h, fcd_ctc_score_*) next to the search it scores, on one GPU: BASELINE config 2
(4096 x 4000 x 5, beam 5, threshold 0.1).

    python tools/probe_score.py [--reps 2] [--out FILE]

Milliseconds (host clock around work that ends in a device synchronise, best of --reps after a warm-up): the beam search
alone; scoring hypothesis 0 of every read at band 64 / 16 / exact; the 5-best search; scoring its 5 hypotheses per read
at band 64.  One JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import fast_ctc_decode_amd as fcd
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_parity import gen_batch

    x = torch.from_numpy(gen_batch(2024, 4096, 4000, 5)).cuda()
    row = {"shape": "config 2", "reads": 4096, "T": 4000}
    row["search_ms"] = best(lambda: fcd.beam_search_batch_raw(x, 5, 0.1), args.reps)
    r = fcd.beam_search_batch_raw(x, 5, 0.1)
    for band in (64, 16, 0):
        row["score_hyp0_%s_ms" % ("band%d" % band if band else "exact")] = best(lambda: r.ctc_score(x, band=band), args.reps)
    row["search_5best_ms"] = best(lambda: fcd.beam_search_nbest_batch_raw(x, 5, 5, 0.1), args.reps)
    nb = fcd.beam_search_nbest_batch_raw(x, 5, 5, 0.1)
    row["score_5hyp_band64_ms"] = best(lambda: nb.ctc_score(x, band=64), args.reps)
    row["mean_labels"] = float(r.out_len.float().mean())
    row["ratio_band64_to_search"] = row["score_hyp0_band64_ms"] / row["search_ms"]
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
