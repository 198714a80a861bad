"""CRF scoring and forced alignment (include/fcd.h, fcd_crf_score_* / fcd_crf_align_*) next to the search whose result
they read and to the CTC walks at the same bands, on one GPU, every figure from one run:

    python tools/probe_crf_lattice.py [--reads 4096] [--large-reads 256] [--out FILE]

  BASELINE config 4's shape (4096 x 4000 x 4 x 5, beam 5): the CRF beam search alone, crf_score and crf_align at bands 16
  and 64; BASELINE config 2 (4096 x 4000 x 5, beam 5, threshold 0.1): ctc_score and ctc_align at the same bands; one large-S
  case that fits memory (256 reads x 4000 x 1024 x 5 in f16: rows gathered from global memory), bands 16 and 64.

Milliseconds, device-resident, a host clock around one call that ends in a device synchronise, the best of 3 after a
warm-up.  One JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=3):
    import torch
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) * 1e3
        best = ms if best is None else min(best, ms)
    return best


def crf_batch(torch, seed, B, T, S, N, dtype):
    """(B, T, S, N) rows that sum to 1 with a blank about as likely as all labels together, made on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((B, T, S, N), dtype=dtype, device="cuda")
    step = max(1, (1 << 26) // (T * S * N))
    for b in range(0, B, step):  # (in slices: the float32 intermediate of the large-S case would not fit twice)
        v = torch.rand((min(step, B - b), T, S, N), generator=g, device="cuda") ** 3
        v[..., 0] *= 4.0
        x[b:b + step] = (v / v.sum(-1, keepdim=True)).to(dtype)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--large-reads", type=int, default=256)
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import fast_ctc_decode_amd as fcd
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_parity import gen_batch

    T = args.rows
    row = {"reads": args.reads, "T": T}
    # config 4's shape
    x = crf_batch(torch, 4, args.reads, T, 4, 5, torch.float32)
    init = torch.rand((args.reads, 4), device="cuda")
    row["crf_search_ms"] = timed(lambda: fcd.crf_beam_search_batch_raw(x, init, 5, 0.0))
    r = fcd.crf_beam_search_batch_raw(x, init, 5, 0.0)
    row["crf_mean_labels"] = float(r.out_len.float().mean())
    for band in (16, 64):
        row["crf_score_band%d_ms" % band] = timed(lambda: r.crf_score(x, init, band=band))
        row["crf_align_band%d_ms" % band] = timed(lambda: r.crf_align(x, init, band=band))
    del x, r
    # config 2, the CTC walks at the same bands
    xc = torch.from_numpy(gen_batch(2024, args.reads, T, 5)).cuda()
    rc = fcd.beam_search_batch_raw(xc, 5, 0.1)
    row["ctc_mean_labels"] = float(rc.out_len.float().mean())
    for band in (16, 64):
        row["ctc_score_band%d_ms" % band] = timed(lambda: rc.ctc_score(xc, band=band))
        row["ctc_align_band%d_ms" % band] = timed(lambda: rc.ctc_align(xc, band=band))
    del xc, rc
    # large S: gathered rows
    n = args.large_reads
    if n > 0:
        xl = crf_batch(torch, 5, n, T, 1024, 5, torch.float16)
        il = torch.rand((n, 1024), device="cuda")
        rl = fcd.crf_beam_search_batch_raw(xl, il, 5, 0.0)
        row["large_reads"], row["large_S"] = n, 1024
        row["large_search_ms"] = timed(lambda: fcd.crf_beam_search_batch_raw(xl, il, 5, 0.0))
        for band in (16, 64):
            row["large_score_band%d_ms" % band] = timed(lambda: rl.crf_score(xl, il, band=band))
            row["large_align_band%d_ms" % band] = timed(lambda: rl.crf_align(xl, il, band=band))
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
