"""Beam-search sessions (include/fcd.h, fcd_beam_session_*) against the one-shot call, on one GPU: BASELINE config 2
(4096 x 4000 x 5, beam 5, threshold 0.1) and config 4's CRF shape (4096 x 4000 x 4 states x 5, beam 5, one-hot init).

    python tools/probe_session.py [--reps 3] [--out FILE]

Per shape, milliseconds for the whole 4000-row read (host clock around work that ends in a device synchronise, best of
--reps after a warm-up): the one-shot launch; a session fed in pushes of 50 / 200 / 400 / 1000 / 4000 rows, without and
with a result per push; result() alone; and re-decoding every 400-row prefix with the one-shot call (what a caller
without sessions does).  One JSON line per shape."""
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


def probe(name, x, one_shot, make_session, reps):
    B, T = x.shape[:2]
    row = {"shape": name, "reads": B, "T": T, "one_shot_ms": best(one_shot(x), reps)}
    s = make_session()
    all_slots = list(range(B))

    def fed(chunk, result):
        def run():
            s.restart(all_slots, *([] if not getattr(s, "_crf", False) else [s._probe_init]))
            for a in range(0, T, chunk):
                s.push(x[:, a:a + chunk], result=result)
        return run

    for chunk in (50, 200, 400, 1000, 4000):
        row["push_%d_ms" % chunk] = best(fed(chunk, False), reps)
        row["push_%d_result_ms" % chunk] = best(fed(chunk, True), reps)
    row["result_ms"] = best(lambda: s.result(), reps)
    row["redecode_400_ms"] = best(lambda: [one_shot(x[:, :a])() for a in range(400, T + 1, 400)], reps)
    s.close()
    o = row["one_shot_ms"]
    row["ratio_push_400"] = row["push_400_ms"] / o
    row["ratio_push_400_result"] = row["push_400_result_ms"] / o
    row["ratio_redecode_400"] = row["redecode_400_ms"] / o
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import fast_ctc_decode_amd as fcd
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_parity import gen_batch

    rows = []
    x = torch.from_numpy(gen_batch(2024, 4096, 4000, 5)).cuda()
    rows.append(probe("config 2", x, lambda v: (lambda: fcd.beam_search_batch_raw(v, 5, 0.1)),
                      lambda: fcd.BeamSearchSession(4096, 5, 4000, 5, 0.1), args.reps))
    print(json.dumps(rows[-1]), flush=True)
    del x
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    x = torch.rand((4096, 4000, 4, 5), generator=g, device="cuda")
    x /= x.sum(-1, keepdim=True)
    init = torch.zeros((4096, 4), device="cuda")
    init[torch.arange(4096), torch.arange(4096) % 4] = 1.0
    init_h = init.cpu().numpy()

    def crf_session():
        s = fcd.CrfBeamSearchSession(4096, 4, 5, init_h, 4000, 5, 0.0)
        s._probe_init = init_h
        return s
    rows.append(probe("config 4 (CRF S=4)", x, lambda v: (lambda: fcd.crf_beam_search_batch_raw(v, init, 5, 0.0)),
                      crf_session, args.reps))
    print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
