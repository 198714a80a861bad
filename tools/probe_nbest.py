"""What the n-best epilogue costs: kernel time (fcd_timing_mean_ms, HIP events around the launches) of one call alone
-- no overlap -- of the existing single-result search next to the n-best search with n_best = 1 and n_best = beam_size,
for BASELINE config 2 (beam 5, 4096 reads), config 3 (beam 32, lane kernel, 8192 reads) and config 4 (CRF beam 5,
S = 4, 4096 reads).  One JSON line per config.

    python tools/probe_nbest.py [2] [3] [4] [--reps K]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import fast_ctc_decode_amd as fcd

CONFIGS = {2: dict(beam=5, thr=0.1, B=4096, crf=False), 3: dict(beam=32, thr=0.1, B=8192, crf=False),
           4: dict(beam=5, thr=0.0, B=4096, crf=True)}


def timed(fn, reps):
    r = fn()
    torch.cuda.synchronize()
    h = r._handle
    h.timing_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return h.timing_mean_ms()[0]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    args = [a for a in args if a != str(reps)]
    fcd.set_overlap(0)
    for c in [int(a) for a in args] or [2, 3, 4]:
        cfg = CONFIGS[c]
        g = torch.Generator(device="cuda")
        g.manual_seed(c)
        beam, thr, B = cfg["beam"], cfg["thr"], cfg["B"]
        if cfg["crf"]:
            x = torch.rand((B, 4000, 4, 5), generator=g, device="cuda", dtype=torch.float32)
            x /= x.sum(-1, keepdim=True)
            init = torch.zeros((B, 4), device="cuda")
            init[torch.arange(B), torch.arange(B) % 4] = 1.0
            calls = {"single": lambda: fcd.crf_beam_search_batch_raw(x, init, beam, thr)}
            for n in (1, beam):
                calls["nbest_%d" % n] = lambda n=n: fcd.crf_beam_search_nbest_batch_raw(x, init, n, beam, thr)
        else:
            x = torch.rand((B, 4000, 5), generator=g, device="cuda", dtype=torch.float32)
            x /= torch.linalg.vector_norm(x, ord=2, dim=-1, keepdim=True)
            calls = {"single": lambda: fcd.beam_search_batch_raw(x, beam, thr)}
            for n in (1, beam):
                calls["nbest_%d" % n] = lambda n=n: fcd.beam_search_nbest_batch_raw(x, n, beam, thr)
        out = {"config": c, "reads": B, "beam": beam, "reps": reps}
        for _ in range(2):  # alternated twice: the spread of the single call is the yardstick
            for name, fn in calls.items():
                out.setdefault(name + "_ms", []).append(round(timed(fn, reps), 4))
        s = min(out["single_ms"])
        for n in (1, beam):
            out["nbest_%d_over_single" % n] = round(min(out["nbest_%d_ms" % n]) / s - 1.0, 4)
        print(json.dumps(out), flush=True)
        del x


if __name__ == "__main__":
    main()
