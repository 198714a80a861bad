"""CRF edge occupancies (include/fcd.h, fcd_crf_occupancy_*) next to crf_score and crf_posterior, which walk the same lattice,
and the CRF-CTC loss (crf_ctc_loss) next to what a ROCm user runs without it: logZ and the labelling's own score as torch
loops of T dependent steps each, and autograd's .backward() through both.  From the same run, on one GPU.

    python tools/probe_crf_occupancy.py [--passes 5] [--torch-passes 2] [--rows 4000] [--reads 4096] [--large-reads 256]
                                        [--loss-reads-s4 8192] [--loss-reads-s64 4096] [--loss-reads-s1024 256] [--out FILE]
    python tools/probe_crf_occupancy.py --wide [--register-only] [--wide-reads 256] [--wide-loss-reads 64] [--root TREE]

--wide times only the shapes of the windows beyond 512 states and of what shares their kernels (wide_shapes below).

Occupancy: BASELINE config 4's shape (4096 x 4000 x 4 states x 5, beam 5), every read's result at band 16 and band 64:
crf_score, crf_posterior and crf_occupancy (into a buffer held across the calls; the call clears the rows it writes), and
one S = 1024 case (f16, gathered rows) at band 16.  The expectation under test: the occupancy walk carries beta alone and
costs less than crf_posterior's walk with its chain values.
Loss: S = 4, 64, 1024 at N = 5 and T = --rows, float32 scores, labellings of 511 random labels (the exact lattice's limit):
crf_ctc_loss forward plus backward, and the torch loops for the same loss; *_over_torch is the loops' time over the call's;
*_max_abs_grad_vs_torch compares the two gradients on 8 reads and *_nan_losses counts those the call refused (a labelling its
read does not support, beyond what rows with one float32 exponent hold: NaN there, and in the difference).
Milliseconds: device events around one device-resident call; after one warm-up call, --passes such calls, the best as *_ms
and all of them as *_all.  A GPU is required; there is no fall-back.  One JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def torch_numerator(torch, x, labels, start):
    """x (B, T, S, N) float32 scores, labels (B, L) int64 in 1 .. N-1, start (B,) -> (B,) float64: ln of the sum over the
    labelling's alignments from `start` of exp(score), one row per step, renormalised"""
    B, T, S, N = x.shape
    L = labels.shape[1]
    nb = N - 1
    sig = [start]
    for k in range(L):
        sig.append((sig[-1] * nb) % S + labels[:, k] - 1)
    sig = torch.stack(sig, dim=1)                                             # (B, L + 1)
    sym = torch.cat([labels, torch.zeros_like(labels[:, :1])], dim=1)         # (B, L + 1); state L emits nothing
    stay_at, adv_at = sig * N, sig * N + sym
    low = -1.0e30
    a = torch.full((B, L + 1), low, dtype=torch.float32, device=x.device)
    a[:, 0] = 0.0
    total = torch.zeros((B,), dtype=torch.float64, device=x.device)
    rows = x.reshape(B, T, S * N).unbind(1)
    pad = torch.full((B, 1), low, dtype=torch.float32, device=x.device)
    for t in range(T):
        stay = a + rows[t].gather(1, stay_at)
        adv = a + rows[t].gather(1, adv_at)
        n = torch.logaddexp(stay, torch.cat([pad, adv[:, :-1]], dim=1))
        c = n.max(dim=1).values.detach()
        total = total + c.double()
        a = n - c[:, None]
    return total + a[:, L].double()


def lattice_cells(T, L):
    """cells of the exact lattice of L labels in T rows: the states of every row's window (the cone)"""
    return sum(min(L, t + 1) - max(0, L - (T - 1 - t)) + 1 for t in range(T))


def wide_shapes(torch, fcd, args, row, put):
    """--wide: the shapes behind INTEGRATION.md section 2p.
    Register-resident, eight states per lane (T = 1000, 495 labels, --wide-reads reads): what ran before the LDS-resident
    walks joined crfp_fwd_kernel<8> and crfp_back_kernel<8, 2, 4> must not get slower -- crf_occupancy at S = 1024 and S = 16,
    crf_posterior and crf_edits at S = 16 (m = 2: the chain tier that runs crfp_back_kernel<8, 2, 4>; S = 1024 is m = 5, three
    states per lane).  Nothing here passes wide=, so the same lines time a build without it (--root).
    LDS-resident (skipped with --register-only): crf_ctc_loss forward and backward and crf_occupancy alone at T = 1600, 800
    labels, S = 1024, --wide-loss-reads reads, and the register walk at its limit, 511 labels in 1022 rows, for the cost per
    lattice cell."""
    N = 5

    def case(S, B, T, L, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        x = torch.softmax(2.0 * torch.randn((B, T, S, N), generator=g, device="cuda"), dim=-1)
        init = torch.rand((B, S), generator=g, device="cuda")
        labels = torch.randint(1, N, (B, L), generator=g, device="cuda").to(torch.uint8)
        lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
        return x, init, labels, lens

    def per_cell(key, B, T, L):
        row[key + "_ns_per_cell"] = round(row[key + "_ms"] * 1e6 / (B * lattice_cells(T, L)), 4)

    B, T, L = args.wide_reads, 1000, 495
    row["reg_shape"] = {"T": T, "labels": L, "reads": B}
    for S in (1024, 16):
        x, init, labels, lens = case(S, B, T, L, S)
        out = torch.zeros((B, 1, T, S, N), dtype=torch.float32, device="cuda")
        put("reg_s%d_occupancy" % S, lambda: fcd.crf_occupancy_batch_raw(x, init, labels, lens, out=out))
        per_cell("reg_s%d_occupancy" % S, B, T, L)
        row["reg_s%d_nan" % S] = int(torch.isnan(fcd.crf_occupancy_batch_raw(x, init, labels, lens, out=out).logp).sum())
        if S == 16:
            put("reg_s16_posterior", lambda: fcd.crf_posterior_batch_raw(x, init, labels, lens))
            put("reg_s16_edits", lambda: fcd.crf_edits_batch_raw(x, init, labels, lens))
        del x, out
        torch.cuda.empty_cache()
    if args.register_only:
        return
    S, B = 1024, args.wide_loss_reads
    for tag, T, L, wide in (("reg511", 1022, 511, False), ("wide", 1600, 800, True)):
        x, init, labels, lens = case(S, B, T, L, T)
        out = torch.zeros((B, 1, T, S, N), dtype=torch.float32, device="cuda")
        row[tag + "_shape"] = {"T": T, "labels": L, "reads": B, "S": S, "cells": lattice_cells(T, L),
                               "states_per_lane": -(-(L + 1) // 64)}
        put(tag + "_occupancy", lambda: fcd.crf_occupancy_batch_raw(x, init, labels, lens, out=out, wide=wide))
        per_cell(tag + "_occupancy", B, T, L)
        put(tag + "_score", lambda: fcd.crf_score_batch_raw(x, init, labels, lens, wide=wide))
        per_cell(tag + "_score", B, T, L)
        row[tag + "_nan"] = int(torch.isnan(fcd.crf_occupancy_batch_raw(x, init, labels, lens, out=out, wide=wide).logp).sum())
        del x, out
        torch.cuda.empty_cache()
        g = torch.Generator(device="cuda").manual_seed(T + 1)
        scores = torch.randn((B, T, S, N), generator=g, device="cuda")

        def loss_and_backward():
            xs = scores.detach().requires_grad_(True)
            fcd.crf_ctc_loss(xs, labels, lens).sum().backward()
            return xs.grad
        put(tag + "_loss", loss_and_backward)
        per_cell(tag + "_loss", B, T, L)
        row[tag + "_loss_nan"] = int(torch.isnan(fcd.crf_ctc_loss(scores, labels, lens)).sum())
        del scores
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", action="store_true", help="only the shapes of INTEGRATION.md section 2p (wide_shapes)")
    ap.add_argument("--register-only", action="store_true", help="--wide: the register-resident shapes alone")
    ap.add_argument("--wide-reads", type=int, default=256)
    ap.add_argument("--wide-loss-reads", type=int, default=64)
    ap.add_argument("--root", default=None, help="import fast_ctc_decode_amd from this tree (another build of the package)")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--torch-passes", type=int, default=2)
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--large-reads", type=int, default=256)
    ap.add_argument("--loss-reads-s4", type=int, default=8192)
    ap.add_argument("--loss-reads-s64", type=int, default=4096)
    ap.add_argument("--loss-reads-s1024", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.root:
        sys.path.insert(0, os.path.abspath(args.root))
    import torch

    import fast_ctc_decode_amd as fcd
    from probe_crf_lattice import crf_batch
    from probe_crf_marginals import torch_logz

    if not torch.cuda.is_available():
        raise SystemExit("probe_crf_occupancy needs the GPU")
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

    def put(name, fn, passes=None):
        ms = timed(fn, passes or args.passes)
        row[name + "_ms"], row[name + "_all"] = min(ms), ms

    def finish():
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")

    if args.wide:
        row = {"passes": args.passes, "package": os.path.dirname(os.path.abspath(fcd.__file__))}
        wide_shapes(torch, fcd, args, row, put)
        return finish()

    # ---- occupancy next to score and posterior ----
    for tag, S, B, dtype, bands in (("config4", 4, args.reads, torch.float32, (16, 64)),
                                    ("s1024", 1024, args.large_reads, torch.float16, (16,))):
        if B <= 0:
            continue
        x = crf_batch(torch, 4 if S == 4 else 5, B, T, S, N, dtype)
        init = torch.rand((B, S), device="cuda")
        r = fcd.crf_beam_search_batch_raw(x, init, 5, 0.0)
        row[tag + "_reads"], row[tag + "_mean_labels"] = B, float(r.out_len.float().mean())
        out = torch.zeros((B, 1, T, S, N), dtype=torch.float32, device="cuda")
        for band in bands:
            key = "%s_band%d" % (tag, band)
            put(key + "_score", lambda: r.crf_score(x, init, band=band))
            put(key + "_posterior", lambda: r.crf_posterior(x, init, band=band))
            put(key + "_occupancy", lambda: fcd.crf_occupancy_batch_raw(x, init, r.labels, r.out_len, None, r.path, band, out=out))
            row[key + "_occupancy_over_posterior"] = round(row[key + "_occupancy_ms"] / row[key + "_posterior_ms"], 3)
            row[key + "_occupancy_over_score"] = round(row[key + "_occupancy_ms"] / row[key + "_score_ms"], 3)
        row[tag + "_max_abs_row_sum_error"] = float((out[:16, 0].sum(dim=(2, 3)) - 1.0).abs().max())
        del x, r, out
        torch.cuda.empty_cache()

    # ---- the loss next to the torch loops ----
    L = min(511, T)
    for S, B in ((4, args.loss_reads_s4), (64, args.loss_reads_s64), (1024, args.loss_reads_s1024)):
        if B <= 0:
            continue
        tag = "loss_s%d" % S
        row[tag + "_reads"], row[tag + "_labels"] = B, L
        g = torch.Generator(device="cuda").manual_seed(S)
        x = 2.0 * torch.randn((B, T, S, N), generator=g, device="cuda")
        labels = torch.randint(1, N, (B, L), generator=g, device="cuda").to(torch.uint8)
        lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
        nb = N - 1
        s = torch.arange(S, device="cuda")
        d = torch.stack([s] + [(s * nb) % S + j for j in range(nb)], dim=1)

        def loss_and_backward():
            xs = x.detach().requires_grad_(True)
            fcd.crf_ctc_loss(xs, labels, lens).sum().backward()
            return xs.grad
        put(tag, loss_and_backward)
        start = fcd.crf_transition_probs_batch_raw(x).init.argmax(dim=1)

        def torch_once(xx, lab, st):
            xs = xx.detach().requires_grad_(True)
            (torch_logz(torch, xs, d) - torch_numerator(torch, xs, lab.long(), st)).sum().backward()
            return xs.grad
        try:
            put(tag + "_torch", lambda: torch_once(x, labels, start), args.torch_passes)
            row[tag + "_over_torch"] = round(row[tag + "_torch_ms"] / row[tag + "_ms"], 2)
        except torch.cuda.OutOfMemoryError:  # (autograd keeps every step's intermediates: several times the scores)
            row[tag + "_torch_ms"] = None
            row[tag + "_torch_note"] = "out of memory: not measured"
        torch.cuda.empty_cache()
        nsmall = min(B, 8)
        xs = x[:nsmall].detach().requires_grad_(True)
        few = fcd.crf_ctc_loss(xs, labels[:nsmall], lens[:nsmall])
        row[tag + "_nan_losses"] = "%d of %d" % (int(torch.isnan(few).sum()), nsmall)  # (reads whose lattice the walks lost)
        few.sum().backward()
        row[tag + "_max_abs_grad_vs_torch"] = float((xs.grad - torch_once(x[:nsmall], labels[:nsmall], start[:nsmall])).abs().max())
        del x, xs
        torch.cuda.empty_cache()
    finish()


if __name__ == "__main__":
    main()
