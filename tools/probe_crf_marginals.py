"""The CRF edge marginals (include/fcd.h, fcd_crf_marginals_*) next to crf_transition_probs -- the backward half alone, on
the same tree -- and next to what a ROCm user runs without the function: logZ as a torch loop of T dependent logsumexp
steps and autograd's .backward() through it.  From the same run, on one GPU.

    python tools/probe_crf_marginals.py [--passes 5] [--torch-passes 2] [--rows 4000] [--reads-s4 8192] [--reads-s64 4096]
                                        [--reads-s1024 256] [--out FILE]

Shapes: S = 4, 64 and 1024 at N = 5, T = --rows, the read counts of tools/probe_crf_transitions.py.  Per shape: float16 and
float32 scores in the source layout, with and without emit; crf_logz forward plus backward (the marginals call, then the
product with grad_out).  Milliseconds: device events around one device-resident call; after one warm-up call, --passes such
calls, the best as *_ms and all of them as *_all.  Bytes of the marginals call: the T S N scores read once, the float32
T S N buffer written by the backward pass, read and written again by the forward pass (*_tbps, *_hbm_share against the 8.0
TB/s peak); *_over_transitions is the call's time over crf_transition_probs' (float32 probabilities) on the same input, and
*_bytes_over_transitions the same ratio of the bytes -- the expectation under test is that the two agree.  The torch loop
runs on float32 scores; *_over_torch is its time over crf_logz's forward plus backward.  A GPU is required; there is no
fall-back.  One JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12


def torch_logz(torch, x, d):
    """x (B, T, S, N) float32 scores, d (S, N) destinations -> logz (B,): the recurrence, one row per step, renormalised"""
    B, T, S, N = x.shape
    beta = torch.zeros((B, S), dtype=torch.float32, device=x.device)
    logz = torch.zeros((B,), dtype=torch.float64, device=x.device)
    flat = d.reshape(-1)
    rows = x.unbind(1)  # (one stack in the backward pass, not a full-size gradient per row)
    for t in range(T - 1, -1, -1):
        b = torch.logsumexp(rows[t] + beta[:, flat].reshape(B, S, N), dim=2)
        c = b.max(dim=1).values.detach()
        logz = logz + c.double()
        beta = b - c[:, None]
    return logz + torch.logsumexp(beta, dim=1).double()


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
        raise SystemExit("probe_crf_marginals needs the GPU")
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
        elems = B * T * S * N
        for in_name, x in (("f16", x16), ("f32", x32)):
            in_bytes = 2 if in_name == "f16" else 4
            key = "%s_%sin" % (tag, in_name)
            ms = timed(lambda: fcd.crf_transition_probs_batch_raw(x), args.passes)
            row[key + "_transitions_ms"], row[key + "_transitions_all"] = min(ms), ms
            for emit in (True, False):
                k2 = key + ("_marginals" if emit else "_marginals_noemit")
                ms = timed(lambda: fcd.crf_marginals_batch_raw(x, emit=emit), args.passes)
                nbytes = elems * (in_bytes + 3 * 4)
                row[k2 + "_ms"], row[k2 + "_all"] = min(ms), ms
                row[k2 + "_tbps"] = round(nbytes / (min(ms) * 1e-3) / 1e12, 3)
                row[k2 + "_hbm_share"] = round(nbytes / (min(ms) * 1e-3) / HBM_PEAK, 3)
                row[k2 + "_over_transitions"] = round(min(ms) / row[key + "_transitions_ms"], 3)
            row[key + "_bytes_over_transitions"] = round((in_bytes + 12) / (in_bytes + 4), 3)

            def logz_and_backward():
                xs = x.detach().requires_grad_(True)
                fcd.crf_logz(xs).sum().backward()
                return xs.grad
            ms = timed(logz_and_backward, args.passes)
            row[key + "_logz_backward_ms"], row[key + "_logz_backward_all"] = min(ms), ms

        # the same quantity from a torch loop and autograd, and the two gradients side by side
        def torch_once(xx):
            xs = xx.detach().requires_grad_(True)
            torch_logz(torch, xs, d).sum().backward()
            return xs.grad
        try:
            ms = timed(lambda: torch_once(x32), args.torch_passes)
            row[tag + "_torch_ms"], row[tag + "_torch_all"] = min(ms), ms
            row[tag + "_f32in_logz_backward_over_torch"] = round(min(ms) / row[tag + "_f32in_logz_backward_ms"], 2)
        except torch.cuda.OutOfMemoryError:  # (autograd keeps every step's intermediates: several times the scores)
            row[tag + "_torch_ms"] = None
            row[tag + "_torch_note"] = "out of memory: not measured"
        torch.cuda.empty_cache()
        nsmall = min(B, 16)
        xs = x32[:nsmall].detach().requires_grad_(True)
        fcd.crf_logz(xs).sum().backward()
        row[tag + "_max_abs_grad_vs_torch"] = float((xs.grad - torch_once(x32[:nsmall])).abs().max())
        r = fcd.crf_marginals_batch_raw(x32[:nsmall])
        assert int(r.status.max()) == 0
        row[tag + "_max_abs_row_sum_error"] = float((r.emit.sum(dim=2) - 1.0).abs().max())
        del x32, x16, r, xs
        torch.cuda.empty_cache()
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
