"""CTC forced alignment (include/fcd.h, fcd_ctc_align_*) next to the scoring call that walks the same lattice and the
search whose result both read, on one GPU: BASELINE config 2 (4096 x 4000 x 5, beam 5, threshold 0.1).

    python tools/probe_align.py [--reps 20] [--reads 4096] [--exact-reads 256] [--out FILE]

Milliseconds (host clock around --inner back-to-back device-resident calls that end in one device synchronise, divided
by --inner; the median of --reps such windows after a warm-up, with the smallest and largest as *_min / *_max):
the beam search alone; aligning and scoring hypothesis 0 of every read at band 16 and band 64, from the same run; the
exact lattice on the first --exact-reads reads; the back-pointer bytes one banded call writes.  One JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, inner):
    """-> (median, min, max) ms per call over `reps` windows of `inner` calls each"""
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3 / inner)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--exact-reads", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import fast_ctc_decode_amd as fcd
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_parity import gen_batch

    T = 4000
    x = torch.from_numpy(gen_batch(2024, args.reads, T, 5)).cuda()
    row = {"shape": "config 2", "reads": args.reads, "T": T, "reps": args.reps, "inner": args.inner}

    def put(name, fn, inner=args.inner):
        row[name + "_ms"], row[name + "_min"], row[name + "_max"] = timed(fn, args.reps, inner)
    put("search", lambda: fcd.beam_search_batch_raw(x, 5, 0.1))
    r = fcd.beam_search_batch_raw(x, 5, 0.1)
    for band in (16, 64):
        put("align_band%d" % band, lambda: r.ctc_align(x, band=band))
        put("score_band%d" % band, lambda: r.ctc_score(x, band=band))
        row["ratio_band%d" % band] = row["align_band%d_ms" % band] / row["score_band%d_ms" % band]
        # 4 band + 3 states at most: 2 bits a slot, 64 bytes a row up to 254 states, 128 up to 510
        row["backpointer_bytes_band%d" % band] = args.reads * T * (64 if 4 * band + 5 <= 256 else 128)
    n = min(args.exact_reads, args.reads)
    if n > 0:
        xe = x[:n]
        re_ = fcd.beam_search_batch_raw(xe, 5, 0.1)
        row["exact_reads"] = n
        put("align_exact", lambda: re_.ctc_align(xe), 2)
        put("score_exact", lambda: re_.ctc_score(xe), 2)
    row["mean_labels"] = float(r.out_len.float().mean())
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
