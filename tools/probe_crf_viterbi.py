"""The CRF Viterbi search (include/fcd.h, fcd_crf_viterbi_search_*) next to crf_beam_search at beam 5 and crf_greedy_search,
from the same run, on one GPU.

    python tools/probe_crf_viterbi.py [--passes 5] [--reads 4096] [--mid-reads 256] [--large-reads 64] [--out FILE]

Three shapes: BASELINE config 4's (4096 x 4000 x 4 states x 5, float32), S = 64 (float32; crf_greedy_search runs on
crf_greedy_kernel there, the serial walk) and S = 1024 (float16).  Milliseconds: the host clock around
one device-resident call and a device synchronise; after one warm-up call, --passes such calls: the best of them as *_ms,
all of them as *_all (their spread is the run-to-run margin).  --package-root DIR imports fast_ctc_decode_amd from another
tree (a build of the parent commit, which has no Viterbi search: its columns are left out).  One JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--mid-reads", type=int, default=256)
    ap.add_argument("--large-reads", type=int, default=64)
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch

    import fast_ctc_decode_amd as fcd
    from probe_crf_lattice import crf_batch

    viterbi = getattr(fcd, "crf_viterbi_search_batch_raw", None)
    T = args.rows
    row = {"T": T, "passes": args.passes, "package": os.path.abspath(args.package_root), "viterbi": viterbi is not None}

    def put(name, fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.passes):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append(round((time.perf_counter() - t) * 1e3, 3))
        row[name + "_ms"], row[name + "_all"] = min(ms), ms

    for tag, seed, B, S, dtype in (("config4", 4, args.reads, 4, torch.float32), ("s64", 6, args.mid_reads, 64, torch.float32),
                                   ("s1024_f16", 5, args.large_reads, 1024, torch.float16)):
        if B <= 0:
            continue
        x = crf_batch(torch, seed, B, T, S, 5, dtype)
        init = torch.rand((B, S), device="cuda")
        row[tag + "_reads"] = B
        put(tag + "_beam5", lambda: fcd.crf_beam_search_batch_raw(x, init, 5, 0.0))
        if dtype == torch.float32 or S > 8:
            put(tag + "_greedy", lambda: fcd.crf_greedy_search_batch_raw(x, init))
        if viterbi is not None:
            put(tag + "_viterbi", lambda: viterbi(x, init))
            put(tag + "_viterbi_qual", lambda: viterbi(x, init, qual=True))
            row[tag + "_viterbi_over_beam5"] = round(row[tag + "_viterbi_ms"] / row[tag + "_beam5_ms"], 3)
            v, g = viterbi(x, init), fcd.crf_greedy_search_batch_raw(x, init)
            row[tag + "_mean_labels"] = float(v.out_len.float().mean())
            row[tag + "_mean_labels_greedy"] = float(g.out_len.float().mean())
            row[tag + "_mean_logp"] = float(v.logp.mean())
            del v, g
        del x, init
        torch.cuda.empty_cache()
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
