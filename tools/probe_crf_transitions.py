"""The CRF transition probabilities (include/fcd.h, fcd_crf_transition_probs_*) next to the same recurrence written as a torch
loop -- T dependent logsumexp steps, what a ROCm user runs without this function -- from the same run, on one GPU.

    python tools/probe_crf_transitions.py [--passes 5] [--torch-passes 2] [--rows 4000] [--reads-s4 8192] [--reads-s64 4096]
                                          [--reads-s1024 256] [--out FILE]

Shapes: S = 4, 64 and 1024 at N = 5, T = --rows, batch sizes that fill the chip (one wavefront per read; 256 CUs hold 2048
to 8192 of them).  Per shape: float16 and float32 scores, float32 and float16 probabilities, both score layouts.
Milliseconds: device events around one device-resident call; after one warm-up call, --passes such calls, the best as *_ms
and all of them as *_all.  Bytes: the T S N scores read and the T S N probabilities written per read, nothing else
(*_tbps, and *_hbm_share against the 8.0 TB/s peak).  The torch loop runs on the float32 scores in the source layout and
writes float32 probabilities; *_over_torch is torch's time over the walk's on the same input.  A GPU is required; there is no
fall-back.  One JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12


def torch_loop(torch, x, d):
    """x (B, T, S, N) float32 scores, d (S, N) destinations -> (probs, init, logz): the recurrence, one row per step"""
    B, T, S, N = x.shape
    beta = torch.zeros((B, S), dtype=torch.float32, device=x.device)
    probs = torch.empty_like(x)
    logz = torch.zeros((B,), dtype=torch.float64, device=x.device)
    flat = d.reshape(-1)
    for t in range(T - 1, -1, -1):
        y = x[:, t] + beta[:, flat].reshape(B, S, N)
        b = torch.logsumexp(y, dim=2)
        probs[:, t] = torch.exp(y - b[:, :, None])
        c = b.max(dim=1).values
        logz += c.double()
        beta = b - c[:, None]
    z = torch.logsumexp(beta, dim=1)
    return probs, torch.exp(beta - z[:, None]), logz + z.double()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--torch-passes", type=int, default=2)
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--reads-s4", type=int, default=8192)
    ap.add_argument("--reads-s64", type=int, default=4096)
    ap.add_argument("--reads-s1024", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    import fast_ctc_decode_amd as fcd

    if not torch.cuda.is_available():
        raise SystemExit("probe_crf_transitions needs the GPU")
    T, N = args.rows, 5
    row = {"T": T, "N": N, "passes": args.passes, "torch_passes": args.torch_passes}

    def timed(fn, passes):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(passes):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1), 3))
        return ms

    for S, B in ((4, args.reads_s4), (64, args.reads_s64), (1024, args.reads_s1024)):
        if B <= 0:
            continue
        tag = "s%d" % S
        row[tag + "_reads"] = B
        g = torch.Generator(device="cuda").manual_seed(S)
        x32 = 2.0 * torch.randn((B, T, S, N), generator=g, device="cuda")
        x16 = x32.half()
        nb = N - 1
        s = torch.arange(S, device="cuda")
        d = torch.stack([s] + [(s * nb) % S + j for j in range(nb)], dim=1)
        for in_name, x in (("f16", x16), ("f32", x32)):
            for out_name in ("f32", "f16"):
                for layout in ("source", "dest"):
                    key = "%s_%sin_%sout_%s" % (tag, in_name, out_name, layout)
                    ms = timed(lambda: fcd.crf_transition_probs_batch_raw(x, layout=layout, out_dtype="float16" if out_name == "f16" else "float32"),
                               args.passes)
                    nbytes = B * T * S * N * ((2 if in_name == "f16" else 4) + (2 if out_name == "f16" else 4))
                    row[key + "_ms"], row[key + "_all"] = min(ms), ms
                    row[key + "_tbps"] = round(nbytes / (min(ms) * 1e-3) / 1e12, 3)
                    row[key + "_hbm_share"] = round(nbytes / (min(ms) * 1e-3) / HBM_PEAK, 3)
        # the same recurrence as a torch loop, and the two results side by side
        ms = timed(lambda: torch_loop(torch, x32, d), args.torch_passes)
        row[tag + "_torch_ms"], row[tag + "_torch_all"] = min(ms), ms
        row[tag + "_f32in_f32out_source_over_torch"] = round(min(ms) / row[tag + "_f32in_f32out_source_ms"], 2)
        row[tag + "_f16in_f16out_source_over_torch"] = round(min(ms) / row[tag + "_f16in_f16out_source_ms"], 2)
        r = fcd.crf_transition_probs_batch_raw(x32[:64])
        p, i, z = torch_loop(torch, x32[:64], d)
        row[tag + "_max_abs_p_vs_torch"] = float((r.probs - p).abs().max())
        row[tag + "_max_abs_logz_vs_torch"] = float((r.logz - z).abs().max())
        assert int(r.status.max()) == 0
        del x32, x16, r, p, i, z
        torch.cuda.empty_cache()
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
