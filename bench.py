#!/usr/bin/env python
"""bench.py -- the driver's benchmark contract for the MI355X-native CTC decoder.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one pass of the hot path -- search::beam_search (beam_size 5, beam_cut_threshold 0.1,
collapse_repeats) over one batch of 4096 synthetic reads of T=4000 x N=5 f32 posteriors per GPU
(BASELINE.json configs[1]; `--config 3` / `--config 4` select configs[2]'s per-rank shard -- beam 32, 8192
reads -- and configs[3], the CRF search, under the same contract) -- with the posteriors already resident
in HBM when the timed region starts.  Reads are independent, so N GPUs decode N independent shards (weak scaling, no collective
inside the search); for N > 1 each step ends with ONE RCCL gather of the decoded
(labels, path, lengths) to rank 0 over xGMI, inside the timed region.

Rank 0 prints ONE JSON line.  `value` is whole-job reads/s = N * batch * K / max-over-ranks time.
`roofline` prices the beam-search kernel against HBM bandwidth with ALGORITHMIC bytes
(T*N*4 in + 5 bytes per emitted label out) over the kernel's own duration measured
with HIP events on the launch stream.  `cpu_baseline` is the CPU oracle (a C restatement of the
reference's Rust, NOT the Rust itself) timed on this box's host cores on a bounded sample, whose
outputs are also compared with the GPU's.  `e2e` (N = 1) is what a caller holding HOST numpy arrays gets from
the compiled module's batch function -- upload, search, packed download and Python objects, pipelined in
chunks -- with array paths and with the reference's list[int] paths; it is never `value`.

A plain run does only what `value` needs: it sets up, warms up, times the K steps and prints the line.  `cpu_baseline`,
`e2e`, `roofline`, the viterbi rooflines, the tie instrument and the other tie order's timing take runs of their own and
are measured only with `--full` (null otherwise).  `--dump-outputs DIR` writes what the last timed step returned
(dump_outputs()); the inputs are seeded, so two builds given the same arguments can be compared array for array.
"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

T, N, BEAM, THR = 4000, 5, 5, 0.1
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s; 6.29 measured copy)

# BASELINE.json configs that fit this contract (one search over one batch per step, T = 4000, N = 5).  The
# default -- what `value` is quoted on -- is config 2 (configs[1]); `--config 3` is the multi-GPU config's
# per-rank shard (64k reads over 8 ranks = 8192 per rank, beam 32), `--config 4` the CRF search.
CONFIGS = {
    2: dict(beam=5, thr=0.1, batch=4096, seed=1, crf=False, overlap=4, kernel_prefix="beam_wave_kernel<5, 6, 2, 0",
            kernel_name="beam_wave_kernel (two reads per wavefront)", baseline="BASELINE.json configs[1]"),
    3: dict(beam=32, thr=0.1, batch=8192, seed=2, crf=False, compare_all=True, overlap=4, kernel_prefix="beam_lane_kernel<5, 2",
            kernel_name="beam_lane_kernel (one beam entry per lane, two reads per wavefront)",
            baseline="BASELINE.json configs[2]: 64k reads sharded over 8 GPUs = 8192 per rank"),
    4: dict(beam=5, thr=0.0, batch=4096, seed=3, crf=True, overlap=4, kernel_prefix="beam_wave_kernel<5, 6, 2, 4",
            kernel_name="beam_wave_kernel (CRF, 4 states, two reads per wavefront)", baseline="BASELINE.json configs[3]"),
    # BASELINE.json configs[4]: the 2-D pair consensus (src/duplex.rs); the metric is pairs/s, `--mode` picks the log-add
    5: dict(beam=5, thr=0.1, batch=1024, seed=4, crf=False, duplex=True, T=2000, band=64, overlap=4,
            kernel_prefix="duplex_slots_kernel<", kernel_name="duplex_slots_kernel (one pair per wavefront, live nodes in LDS slots)",
            baseline="BASELINE.json configs[4]"),
}


def make_batch(seed, n_reads):
    """reference-style rows (tests/test_decode.py:15-17), seeded."""
    rng = np.random.default_rng(seed)
    x = rng.random((n_reads * T, N), dtype=np.float32)
    x /= np.linalg.norm(x, ord=2, axis=1, keepdims=True)
    return x.reshape(n_reads, T, N).astype(np.float32)


def make_batch_peaky(seed, n_reads):
    """SURVEY.md 8d's second, clearly labelled set: peaky softmax rows (logits ~ 4*N(0,1)), the shape
    real basecaller posteriors have -- most symbols fall under beam_cut_threshold.  NOT the metric's
    input; `--data peaky` exists to show how much of the reference-style figure is its worst-case density."""
    rng = np.random.default_rng(seed)
    z = 4.0 * rng.standard_normal((n_reads * T, N), dtype=np.float32)
    z -= z.max(axis=1, keepdims=True)
    np.exp(z, out=z)
    z /= z.sum(axis=1, keepdims=True)
    return z.reshape(n_reads, T, N).astype(np.float32)


DUMP_BYTES = 56 << 20  # under the 64 MB a dump may take
DUMP_READS = 1024


def dump_outputs(dirname, rc):
    """--dump-outputs: the host copy `rc` of what the last timed step returned, as DIR/<name>.npy.  out_len and status
    are written whole (float64).  labels and qual (float32) and path (float64) are (reads, positions) arrays: they are
    written for a fixed sample of reads (default_rng(0), at most DUMP_READS, in read order; all of them when the batch is
    that small), with every position at or past the read's out_len set to -1, since what lies there is not part of the
    result.  Returns {name: shape}."""
    os.makedirs(dirname, exist_ok=True)
    lens = np.asarray(rc.out_len).astype(np.int64)
    B = len(lens)
    rows = {k: np.asarray(getattr(rc, k)) for k in ("labels", "path", "qual") if getattr(rc, k) is not None}
    per_read_bytes = sum(8 * a.shape[1] if k == "path" else 4 * a.shape[1] for k, a in rows.items())
    n = int(max(1, min(B, DUMP_READS, (DUMP_BYTES - 16 * B) // max(per_read_bytes, 1))))
    pick = np.arange(B) if n == B else np.sort(np.random.default_rng(0).choice(B, n, replace=False))
    out = {"out_len": lens.astype(np.float64), "status": np.asarray(rc.status).astype(np.float64)}
    for k, a in rows.items():
        valid = np.arange(a.shape[1])[None, :] < lens[pick, None]
        v = a[pick].astype(np.float64 if k == "path" else np.float32)
        v[~valid] = -1
        out[k] = v
    for k, a in out.items():
        np.save(os.path.join(dirname, k + ".npy"), a)
    return {k: list(a.shape) for k, a in out.items()}


def cpu_baseline(cfg, x_host, init_host, gpu_labels, gpu_path, gpu_len, budget_s):
    """Times the oracle (C restatement of src/search.rs -- NOT the Rust) on this box's host cores
    on a bounded sample of the same workload and checks the GPU's outputs against it.

    os.cpu_count() over-reports what a container may actually use, so the thread count is found
    empirically: short probes at 1, 2, 4, ... threads until throughput stops improving; the timed
    run uses the best count and ~budget_s seconds of wall time."""
    from oracle import oracle

    # The checker follows the product's rule for EQUAL probabilities above 20 candidates (FCD_TIE_ORDER / fcd.tie_order();
    # FCD_PDQ178_STD_FORM): a correct run reports 0 mismatches under either order (r05: the oracle always sorted its own
    # default way, and `FCD_TIE_ORDER=stable python bench.py` printed 2 "mismatches" on reads 1198 and 3588).
    import fast_ctc_decode_amd as fcd
    from fast_ctc_decode_amd import _native as nat
    oracle.lib.fcdo_set_unstable_sort(0 if fcd.tie_order() == "stable" else 1)
    oracle.lib.fcdo_set_pdq_std_form(int(nat.load().fcd_debug_get_pdq178_std_form()) & 3)

    beam, thr = cfg["beam"], cfg["thr"]
    n_avail = x_host.shape[0]
    max_threads = os.cpu_count() or 1
    if cfg["crf"]:
        # the oracle has no threaded CRF driver: one thread, a handful of reads
        n = 0
        mism = 0
        t0 = time.perf_counter()
        while n < min(n_avail, 64) and time.perf_counter() - t0 < budget_s:
            st, labels, path, _ = oracle.crf_beam_search_ambiguous(x_host[n], init_host[n], beam, thr)
            L = len(labels)
            ok = st == 0 and int(gpu_len[n]) == L and np.array_equal(gpu_labels[n, :L], labels) \
                and np.array_equal(gpu_path[n, :L].astype(np.int64), path)
            mism += 0 if ok else 1
            n += 1
        dt = time.perf_counter() - t0
        return {"value": n / dt, "unit": "reads/s", "cores": 1, "kind": "port",
                "sample": "first %d reads of rank 0's batch (T=%d S=4 N=%d beam=%d thr=%.1f), oracle C restatement of "
                          "src/search.rs crf_beam_search, 1 thread, %.1f s" % (n, T, N, beam, thr, dt),
                "single_thread_reads_per_s": n / dt, "gpu_vs_oracle_mismatches": mism, "gpu_vs_oracle_compared": n}

    def run(n, threads, passes=1, out=None):
        out = out or oracle.batch_outputs(n, T)
        t0 = time.perf_counter()
        res = oracle.beam_search_batch(x_host[:n], beam, thr, True, threads, n_passes=passes, out=out)
        return n * passes / (time.perf_counter() - t0), res

    rate1, _ = run(32 if beam <= 8 else 8, 1)
    best_rate, best_threads = rate1, 1
    threads = 2
    while threads <= max_threads:
        n = min(n_avail, max(64, 4 * threads))
        rate, _ = run(n, threads)
        if rate > best_rate * 1.10:
            best_rate, best_threads = rate, threads
            threads *= 2
        else:
            break
    n = int(min(n_avail, max(64, best_rate * budget_s)))
    passes = int(max(1, min(256, best_rate * budget_s / n)))
    out = oracle.batch_outputs(n, T)  # pre-touched: page faults stay out of the timed call
    t0 = time.perf_counter()
    labels, path, lens, status = oracle.beam_search_batch(x_host[:n], beam, thr, True, best_threads,
                                                          n_passes=passes, out=out)
    dt = time.perf_counter() - t0

    def compare(first, labels, path, lens, status):
        bad = 0
        for j in range(len(lens)):
            i = first + j
            L = int(lens[j])
            ok = status[j] == 0 and int(gpu_len[i]) == L \
                and np.array_equal(gpu_labels[i, :L], labels[j, :L]) \
                and np.array_equal(gpu_path[i, :L].astype(np.int64), path[j, :L])
            bad += 0 if ok else 1
        return bad

    mism = compare(0, labels, path, lens, status)
    n_compared = n
    if cfg.get("compare_all") and n < n_avail:
        # (outside the timed sample: the rest of the batch, so that EVERY timed read is checked -- BASELINE config 3's
        # shard is 8192 reads at beam 32, ~20 s of oracle time on a 64-thread host)
        for first in range(n, n_avail, 1024):
            m = min(1024, n_avail - first)
            l2, p2, n2, s2 = oracle.beam_search_batch(x_host[first:first + m], beam, thr, True, best_threads)
            mism += compare(first, l2, p2, n2, s2)
        n_compared = n_avail
    return {
        "value": n * passes / dt, "unit": "reads/s", "cores": best_threads, "kind": "port",
        "sample": "first %d reads of rank 0's batch x %d passes (T=%d N=%d beam=%d thr=%.1f), oracle C "
                  "restatement of src/search.rs, %d pthreads (best of a 1,2,4,.. probe; os.cpu_count()=%d), "
                  "%.1f s" % (n, passes, T, N, beam, thr, best_threads, max_threads, dt),
        "single_thread_reads_per_s": rate1,
        "gpu_vs_oracle_mismatches": mism, "gpu_vs_oracle_compared": n_compared,
        "oracle_tie_order": "stable" if oracle.lib.fcdo_get_unstable_sort() == 0 else "pdq178",
    }


KERNEL_SOURCES = {  # the files a kernel's instruction stream and memory traffic depend on
    "beam_wave_kernel": ("beam_wave.hip", "beam_wave_step.inc", "pdq178.h", "pdq178_wave.h", "pdq178_reg.h", "device_utils.h"),
    "beam_lane_kernel": ("beam_lane.hip", "slab_pool.h", "pdq178.h", "pdq178_wave.h", "pdq178_reg.h", "device_utils.h"),
    "beam_generic_kernel": ("beam_generic.hip", "pdq178.h", "device_utils.h"),
    "viterbi": ("viterbi.hip", "device_utils.h"),
    "crf_greedy": ("viterbi.hip", "device_utils.h"),
    "duplex_kernel": ("duplex.hip", "duplex_math.h", "logadd_fast.h", "glibc235_math.h", "pdq178.h", "device_utils.h"),
    "duplex_slots_kernel": ("duplex_slots.hip", "duplex_math.h", "logadd_fast.h", "glibc235_math.h", "pdq178.h", "device_utils.h"),
    "envelope_kernel": ("envelope.hip", "device_utils.h"),
}


def kernel_source_digest(kernel_prefix=None):
    """{file: md5} of the kernel sources (all of them, or the ones `kernel_prefix` depends on).  Committed counter
    summaries carry the digests of the sources they were taken on, and bench.py quotes them only while those files
    are unchanged: a kernel change without a re-profile gives null, not stale bytes."""
    import hashlib
    csrc = os.path.join(ROOT, "fast_ctc_decode_amd", "csrc")
    files = sorted({f for fs in KERNEL_SOURCES.values() for f in fs})
    if kernel_prefix is not None:
        files = []
        for k, fs in KERNEL_SOURCES.items():
            if kernel_prefix.startswith(k):
                files = list(fs)
    out = {}
    for name in files:
        with open(os.path.join(csrc, name), "rb") as f:
            out[name] = hashlib.md5(f.read()).hexdigest()
    return out


def kernel_occupancy(mangled_substring):
    """What the dispatched instantiation reserves, read off the gfx950 code object inside libfcd_hip.so (so that an
    occupancy regression shows in the driver's own bench line): VGPRs, scratch and LDS bytes per
    wavefront / workgroup, and the wavefronts per SIMD they allow (512 VGPRs per SIMD lane in granules of 8, at most 8
    wavefronts; 160 KiB of LDS per CU over 4 SIMDs).  None when the LLVM tools are missing -- never an exception."""
    import re
    import shutil
    import subprocess
    import tempfile
    try:
        from fast_ctc_decode_amd import _native as nat
        llvm = "/opt/rocm/lib/llvm/bin"
        tmp = tempfile.mkdtemp(prefix="fcd_occ_")
        try:
            subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", nat.LIB_PATH, tmp + "/fat.bin"],
                                  stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            # the section holds one offload bundle per translation unit, back to back
            blob = open(tmp + "/fat.bin", "rb").read()
            magic = b"__CLANG_OFFLOAD_BUNDLE__"
            starts = [m.start() for m in re.finditer(re.escape(magic), blob)] + [len(blob)]
            notes = ""
            for i in range(len(starts) - 1):
                with open(tmp + "/one.bin", "wb") as f:
                    f.write(blob[starts[i]:starts[i + 1]])
                rc = subprocess.call([llvm + "/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                      "--input=" + tmp + "/one.bin", "--output=" + tmp + "/dev.co", "--unbundle"],
                                     stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                if rc == 0 and mangled_substring.split("ILi")[0].encode() in blob[starts[i]:starts[i + 1]]:
                    notes += subprocess.check_output([llvm + "/llvm-readelf", "--notes", tmp + "/dev.co"],
                                                     stderr=subprocess.DEVNULL).decode()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name or mangled_substring not in name.group(1):
                continue
            g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
            vgpr, lds, scratch, wg = g("vgpr_count"), g("group_segment_fixed_size"), g("private_segment_fixed_size"), g("max_flat_workgroup_size")
            by_vgpr = min(8, 512 // max(8, (vgpr + 7) // 8 * 8))
            waves_per_wg = max(1, wg // 64)
            by_lds = (160 * 1024 // lds) * waves_per_wg // 4 if lds else 8
            return {"kernel_symbol": name.group(1)[:96], "vgpr": vgpr, "scratch_bytes": scratch, "lds_bytes_per_workgroup": lds,
                    "wavefronts_per_workgroup": waves_per_wg, "wavefronts_per_simd_by_vgpr": by_vgpr,
                    "wavefronts_per_simd_by_lds": min(8, by_lds), "wavefronts_per_simd": min(by_vgpr, 8, by_lds)}
    except Exception:  # noqa: BLE001  (nothing in the timed script may fail for want of a tool)
        return None
    return None


def digest_matches(recorded, kernel_prefix):
    now = kernel_source_digest(kernel_prefix)
    return bool(now) and isinstance(recorded, dict) and all(recorded.get(k) == v for k, v in now.items())


def e2e_leg(fcd, cfg, x_host, init_host, ref_result, reps=3):
    """What a caller of the reference's surface gets (src/lib.rs:318-365: host numpy in, (str, path) out), outside
    `value`: the compiled module's *_batch function on the HOST batch -- chunked upload || search || packed
    download || Python objects (csrc/hostjob.hip, csrc/pymodule.cpp) -- with array paths and with the
    reference's list[int] paths.  Outputs are compared with the device path's."""
    from fast_ctc_decode_amd import api
    cm = api._compiled()
    B = x_host.shape[0]

    def call(paths):
        if cfg["crf"]:
            return cm.crf_beam_search_batch(x_host, init_host, "NACGT", cfg["beam"], cfg["thr"], paths=paths)
        return cm.beam_search_batch(x_host, "NACGT", cfg["beam"], cfg["thr"], True, paths=paths)

    out = {"unit": "reads/s", "reads": B, "input": "host numpy float32 (pageable), one (B,T,N) array"}
    call("array")  # lanes, arenas and page-locked buffers are allocated by the first job
    res = None
    for mode in ("array", "list"):
        best = None
        for _ in range(reps):
            res = None  # (the previous result is torn down OUTSIDE the timed call: 8 million reference-count decrements
            #              for list paths -- the caller pays them whenever it lets go of a result, not per call)
            t0 = time.perf_counter()
            res = call(mode)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out["paths_" + mode] = B / best
        out["ms_paths_" + mode] = best * 1e3
    want = ref_result.sequences("NACGT", paths="list") if not cfg["crf"] else None
    if want is not None:
        out["identical_to_device_path"] = bool(all(a == b for a, b in zip(res, want)))
    if not cfg["crf"]:
        # the same reads held as float16 -- what basecaller networks emit; the reference would be given an upcast
        # float32 copy (src/lib.rs:182) -- uploaded at half the bytes and converted exactly in the kernel's loads
        # (fcd_batch.dtype).  Compared with the float32 call on the upcast matrix, as the reference would see it.
        xh = x_host.astype(np.float16)
        cm.beam_search_batch(xh, "NACGT", cfg["beam"], cfg["thr"], True, paths="array")
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            res_h = cm.beam_search_batch(xh, "NACGT", cfg["beam"], cfg["thr"], True, paths="array")
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out["float16_input_paths_array"] = B / best
        out["ms_float16_input_paths_array"] = best * 1e3
        n_chk = min(B, 256)
        up = xh[:n_chk].astype(np.float32)
        res_u = cm.beam_search_batch(up, "NACGT", cfg["beam"], cfg["thr"], True, paths="array")
        out["float16_identical_to_upcast_float32"] = bool(all(
            a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(res_h[:n_chk], res_u)))
    return out


def _counting_instantiation(name):
    """beam_wave_kernel<N, GW, RPW, S, AMB, ...> / beam_lane_kernel<N, RPW, AMB, CRF>: the tie-counting (AMB = true)
    instantiations are not the timed kernels."""
    args = [a.strip() for a in name[name.find("<") + 1:name.rfind(">")].split(",")] if "<" in name else []
    if name.startswith("beam_wave_kernel"):
        return len(args) > 4 and args[4] == "true"
    if name.startswith("beam_lane_kernel"):
        return len(args) > 2 and args[2] == "true"
    return False


def pmc_traffic(kernel_prefix):
    """HBM bytes per launch from the newest committed PMC summary (profiles/*_pmc_summary.json,
    produced by tools/profile.sh: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the
    same kernel at the same shape, FETCH_SIZE corrected as MI355X_MICROARCH.md prescribes) -- quoted only
    when the summary was taken on the kernel sources of this tree (kernel_source_digest)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_summary.json")))
    stale = None
    for path in reversed(files):  # newest summary that holds this kernel
        with open(path) as f:
            summ = json.load(f)
        for name, e in summ.get("kernels", {}).items():
            if name.startswith(kernel_prefix) and not _counting_instantiation(name) and "hbm_bytes_per_launch" in e:
                if not digest_matches(summ.get("kernel_source_md5"), kernel_prefix):
                    stale = stale or os.path.basename(path)
                    continue
                return e["hbm_bytes_per_launch"], "%s: %s; %s; %s" % (
                    os.path.basename(path), name, e.get("workload", ""), e.get("fetch_correction_note", ""))
    if stale:
        return None, "no counter summary of the CURRENT kernel sources (newest: %s, taken on other sources); " \
                     "re-run tools/round_profiles.sh" % stale
    return None, None


def valu_issue_roofline(kernel_prefix, kernel_ms, n_simd, clock_hz=2.4e9):
    """The bound the beam kernel actually runs against: VALU instruction issue.  achieved = wavefront-level
    VALU instructions per launch (SQ_INSTS_VALU from the newest committed profiles/*_sq_counters.json of
    this kernel at this shape: tools/profile_sq.sh, rocprofv3 --pmc in its own passes) / the kernel duration
    measured here; peak = one wave64 VALU instruction per SIMD every 2 cycles (SIMD-32,
    MI355X_MICROARCH.md 'v_fma_f32 (wave64): 2 cyc') x SIMDs x 2.4 GHz."""
    import glob
    for path in reversed(sorted(glob.glob(os.path.join(ROOT, "profiles", "*_sq_counters.json")))):
        with open(path) as f:
            d = json.load(f)
        if not digest_matches(d.get("kernel_source_md5"), kernel_prefix):
            continue
        if kernel_prefix in (d.get("kernel") or "") and "SQ_INSTS_VALU" in d.get("counters_per_launch", {}):
            insts = d["counters_per_launch"]["SQ_INSTS_VALU"]
            per_step = d.get("per_wave_step", {})
            achieved = insts / (kernel_ms * 1e-3)
            peak = n_simd * clock_hz / 2.0
            return {
                "bound": "valu_issue", "achieved": achieved, "peak": peak, "unit": "wave64 VALU instructions/s",
                "frac": achieved / peak,
                "source": "%s: SQ_INSTS_VALU %.4g per launch (%s)" % (os.path.basename(path), insts, d.get("workload", "")),
                "per_wavefront_step": {k: round(per_step[k], 1) for k in
                                       ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_WAVE_CYCLES",
                                        "SQ_ACTIVE_INST_ANY", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY") if k in per_step},
                "note": "at 4096 reads only 2 wavefronts share a SIMD: the step time is the wavefront's own dependent "
                        "instruction chain (a lone wavefront per SIMD takes ~87 % as long per step), so the fraction "
                        "rises with the batch (profiles/r02*_cycle_account.jsonl, DESIGN.md 4.1)",
            }
    return None


def viterbi_roofline(fcd, torch, dev, n_reads=16384, reps=20, half=False):
    """The HBM-bound kernel of the path: viterbi_search on n_reads x T x N,
    timed with the C ABI's HIP events.  half: the same reads as float16 -- what basecaller networks emit -- read
    directly by the kernel (fcd_batch.dtype), algorithmic bytes counted at two bytes per posterior."""
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    x = torch.rand((n_reads, T, N), generator=g, device=dev, dtype=torch.float32)
    x /= torch.linalg.vector_norm(x, ord=2, dim=-1, keepdim=True)
    if half:
        x = x.to(torch.float16)
    for _ in range(3):  # (0.3 ms launches: a few of them before the clock is read)
        r = fcd.viterbi_search_batch_raw(x)
    torch.cuda.synchronize()
    h = r._handle
    h.timing_reset()
    for _ in range(reps):
        r = fcd.viterbi_search_batch_raw(x)
    torch.cuda.synchronize()
    ms, calls = h.timing_mean_ms()
    mean_L = float(r.out_len.float().mean())
    bytes_per_read = T * N * (2 if half else 4) + 5.0 * mean_L
    achieved = n_reads * bytes_per_read / (ms * 1e-3) / 1e9
    traffic, note = pmc_traffic("viterbi_stream_kernel<5, 1" if half else "viterbi_stream_kernel<5, 0")
    return {
        "kernel": "viterbi_stream_kernel<5, %s> (search::viterbi_search)" % ("f16" if half else "f32"), "bound": "hbm",
        "input_dtype": "f16" if half else "f32",
        "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
        "traffic": traffic, "traffic_source": note,
        "reads": n_reads, "kernel_ms": ms, "launches_timed": calls,
        "reads_per_s": n_reads / (ms * 1e-3), "algorithmic_bytes_per_read": bytes_per_read,
        "clock": viterbi_clock_note() if not half else None,
    }


def viterbi_clock_note():
    """`kernel_ms` above is the mean of the C ABI's HIP events on the launch stream.  The newest committed
    profiles/*_viterbi_clock_summary.json (tools/viterbi_clock.sh) holds both clocks for the SAME launches of one
    process -- events run 1-2.5 % above the profiler's kernel duration (they bracket the dispatch, not only the
    kernel) -- so a reader can price `frac` by either."""
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_viterbi_clock_summary.json"))):
        best = f
    if not best:
        return None
    try:
        d = json.load(open(best))
        rows = d.get("rocprofv3_kernel_stats_same_process") or []
        prof_ms = float(rows[0]["AverageNs"]) * 1e-6 if rows else None
        ev_ms = float(d["hip_events_under_rocprof"]["mean"])
        return {"source": os.path.relpath(best, ROOT), "kernel_ms_events_same_process": ev_ms,
                "kernel_ms_rocprofv3_same_process": prof_ms,
                "events_over_rocprofv3": (ev_ms / prof_ms) if prof_ms else None}
    except Exception as e:  # a malformed summary must not take the bench line down
        return {"source": os.path.relpath(best, ROOT), "error": str(e)}


def free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(args):
    """`python bench.py --gpus N ...` without a launcher around it: start N ranks of this script through
    torch.distributed.run (one process per GPU, rendezvous on 127.0.0.1) and pass their exit code on.  Fewer than N
    devices: say so and fail (rc 2) -- never a silent smaller run."""
    import subprocess
    if not args.stub:
        import torch
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            sys.stderr.write("bench.py: --gpus %d but this node shows %d GPU(s); nothing was run\n" % (args.gpus, have))
            return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this driver
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def stub_main(args):
    """The distributed skeleton of main() with nothing to decode (TEST ONLY, --stub): gloo on the CPU."""
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (the launcher and the flag must agree)" % (args.gpus, world))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo")
    B = args.batch or CONFIGS[args.config]["batch"]

    def step():
        time.sleep(0.002 * (1 + rank))  # ranks of different speed: the clock must be the slowest one's

    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    if world > 1:
        dist.barrier()
    mine = time.perf_counter() - t0
    t = torch.tensor([mine], dtype=torch.float64)
    allr = [torch.zeros_like(t) for _ in range(world)]
    if world > 1:
        dist.all_gather(allr, t)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    else:
        allr = [t.clone()]
    elapsed = float(t.item())
    if rank == 0:
        print(json.dumps({"metric": "reads/s (T=4000, N=5, beam=%d)" % CONFIGS[args.config]["beam"], "stub": True,
                          "value": world * B * args.steps / elapsed, "unit": "reads/s", "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
                          "scaling": "weak", "ranks": {"world_size": dist.get_world_size() if world > 1 else 1, "backend": "gloo",
                                                       "per_rank_ms_per_step": [float(a.item()) / args.steps * 1e3 for a in allr]},
                          "config": {"baseline_config": args.config, "reads_per_gpu": B}}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def duplex_main(args, cfg, torch, dist, fcd, world, rank, local_rank, dev, distributed):
    """--config 5: duplex::beam_search (src/duplex.rs:443-650) on 1024 pairs of T = 2000 rows, band +-64 around the
    diagonal, beam 5, threshold 0.1 -- the same contract as the 1-D line (a step = one batch of pairs resident in HBM; steps
    overlap on the handle's internal streams unless --overlap 0; `value` = pairs/s over the K timed steps).  Pairs are
    independent: N > 1 runs a shard per rank, no collective in the timed region."""
    from fast_ctc_decode_amd import _native as nat
    Td, band_w, beam, thr = cfg["T"], cfg["band"], cfg["beam"], cfg["thr"]
    B = args.batch or cfg["batch"]
    mode = {"logsumexp": nat.LOGADD_LOGSUMEXP, "max": nat.LOGADD_MAX}[args.mode]
    rng = np.random.default_rng(cfg["seed"] + rank)

    def rows(n):
        x = rng.random((n, N), dtype=np.float32)
        x /= np.linalg.norm(x, ord=2, axis=1, keepdims=True)
        return x.astype(np.float32)

    x1_host = rows(B * Td).reshape(B, Td, N)
    x2_host = rows(B * Td).reshape(B, Td, N)
    i = np.arange(Td)
    env_host = np.stack([np.maximum(0, i - band_w), np.minimum(Td, i + band_w)], 1).astype(np.uint64)
    x1, x2 = torch.from_numpy(x1_host).to(dev), torch.from_numpy(x2_host).to(dev)
    envs = torch.from_numpy(np.broadcast_to(env_host, (B, Td, 2)).copy().view(np.int64)).to(dev)
    torch.cuda.synchronize()
    h = nat.default_handle(local_rank)
    overlap = cfg.get("overlap", 0) if args.overlap is None else max(0, args.overlap)
    if overlap < 2:
        overlap = 0
    h.set_overlap(overlap)

    def step():
        return fcd.beam_search_duplex_batch_raw(x1, x2, envs, beam, thr, True, logadd_mode=mode)

    def join():
        if overlap:
            h.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            h.overlap_join()

    r = None
    for _ in range(max(args.warmup, 1)):
        r = step()
    join()
    torch.cuda.synchronize()
    if overlap:  # (bench main: the caching allocator gets the K sets of result tensors before the clock starts)
        prime = [[torch.empty_like(t) for t in (r.labels, r.out_len, r.status)] for _ in range(args.steps + 1)]
        del prime
    if distributed:
        dist.barrier()
    torch.cuda.synchronize()
    h.timing_reset()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        r = step()
    join()
    torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    k_ms, k_calls = h.timing_mean_ms()
    single_ms = None
    if overlap and args.full:
        h.set_overlap(0)
        h.timing_reset()
        for _ in range(min(args.steps, 3)):
            step()
        torch.cuda.synchronize()
        single_ms = h.timing_mean_ms()[0]
    t_max = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    if distributed:
        dist.all_reduce(t_max, op=dist.ReduceOp.MAX)
    elapsed = float(t_max.item())
    if rank == 0:
        rc = r.cpu()
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, rc)
        ok = int((np.asarray(rc.status) == 0).sum())
        lens = np.asarray(rc.out_len).astype(np.int64)
        mean_L = float(lens.mean())
        # the CPU leg: the oracle (correctly rounded log-add, as the kernels define it) on a bounded sample, a pair per thread
        cpu = None
        if world == 1 and args.full:
            from concurrent.futures import ThreadPoolExecutor
            from oracle import oracle
            omode = (oracle.LOGSUMEXP if args.mode == "logsumexp" else oracle.MAXMODE) | oracle.MATH_CR
            oracle.lib.fcdo_set_unstable_sort(0 if fcd.tie_order() == "stable" else 1)
            threads = min(os.cpu_count() or 1, 32)

            def one(j):
                return oracle.beam_search_duplex(x1_host[j], x2_host[j], "NACGT", env_host, beam, thr, True, omode)

            t1 = time.perf_counter()
            one(0)
            per_pair = time.perf_counter() - t1
            n = int(max(threads, min(B, args.cpu_seconds * threads / max(per_pair, 1e-3))))
            pick = np.linspace(0, B - 1, min(n, B)).astype(np.int64)
            t1 = time.perf_counter()
            with ThreadPoolExecutor(threads) as pool:  # (the C routine runs outside the interpreter lock)
                wants = list(pool.map(one, pick))
            dt = time.perf_counter() - t1
            mism = sum(1 for j, want in zip(pick, wants)
                       if int(rc.status[j]) != 0 or "".join("NACGT"[l] for l in rc.labels[j, :lens[j]]) != want)
            cpu = {"value": len(pick) / dt, "unit": "pairs/s", "cores": threads, "kind": "port",
                   "sample": "%d pairs spread over rank 0's batch (T1=T2=%d N=%d band +-%d beam=%d thr=%.1f, %s), oracle C "
                             "restatement of src/duplex.rs with correctly rounded ln / exp / ln_1p, %d threads (a pair each), "
                             "%.1f s" % (len(pick), Td, N, band_w, beam, thr, args.mode, threads, dt),
                   "single_thread_pairs_per_s": 1.0 / per_pair,
                   "gpu_vs_oracle_mismatches": mism, "gpu_vs_oracle_compared": int(len(pick))}
        bytes_per_pair = 2 * Td * N * 4 + mean_L  # both reads' posteriors in, u8 labels out
        in_flight = k_ms * args.steps / (elapsed * 1e3) if overlap else 1.0  # (bench main: a call's share of the chip)
        k_eff_ms = k_ms / in_flight if overlap else k_ms
        achieved = B * bytes_per_pair / (k_eff_ms * 1e-3) / 1e9
        prefix = "duplex_slots_kernel<%d" % (0 if args.mode == "logsumexp" else 1)
        traffic, traffic_note = pmc_traffic(prefix) if (B == cfg["batch"] and args.full) else (None, None)
        out = {
            "metric": "pairs/s (2-D pair consensus, T=%d, N=5, beam=%d, band +-%d, %s)" % (Td, beam, band_w, args.mode),
            "value": world * B * args.steps / elapsed, "unit": "pairs/s", "n_gpus": world, "steps": args.steps,
            "warmup": max(args.warmup, 1), "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "beam_search_duplex beam_size=%d beam_cut_threshold=%.1f collapse_repeats logadd=%s, "
                                   "batch=%d pairs T1=T2=%d N=5 per GPU (%s), envelope = band +-%d around the diagonal, "
                                   "reference-style rows numpy default_rng(%d+rank)"
                                   % (beam, thr, args.mode, B, Td, cfg["baseline"], band_w, cfg["seed"]),
                       "baseline_config": 5, "pairs_per_gpu": B, "T": Td, "N": N, "beam_size": beam, "beam_cut_threshold": thr,
                       "logadd_mode": args.mode, "kernel": cfg["kernel_name"], "pairs_ok": ok, "mean_labels_per_pair": mean_L,
                       "overlap": overlap, "tie_order": fcd.tie_order(),
                       "parallelism": "pairs sharded x%d, no collective" % world if world > 1 else "single GPU"},
            "full": args.full,
            "roofline": None if not args.full else {
                "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                "traffic": traffic, "traffic_source": traffic_note,
                "kernel": "duplex search (log-space copies + kernel), %.3f ms per call (HIP events)%s, %d pairs x %.0f "
                          "algorithmic B/pair" % (k_ms, " with %.2f calls in flight on average = %.3f ms of the chip per call"
                                                  % (in_flight, k_eff_ms) if overlap else "", B, bytes_per_pair),
                "kernel_ms": k_ms, "launches_timed": k_calls, "launches_in_flight": in_flight,
                "overlap": None if not overlap else {
                    "streams": overlap, "sustained_ms_per_launch": elapsed / args.steps * 1e3,
                    "achieved_one_launch_at_a_time": B * bytes_per_pair / (single_ms * 1e-3) / 1e9 if single_ms else None,
                    "single_launch_ms": single_ms, "single_launch_pairs_per_s": B / (single_ms * 1e-3) if single_ms else None},
                # the search is bound by a serial chain, not by HBM: (band + 1) dependent, correctly rounded log-adds per
                # step and pair -- tools/duplex_account.py prices the kernel against THAT
                "secondary_bound": {"bound": "dependent log-add chain per step", "see": "tools/duplex_account.py -> "
                                    "profiles/*_duplex_account.jsonl (chain_roofline.frac)"},
                "wavefronts_per_simd": B / (torch.cuda.get_device_properties(dev).multi_processor_count * 4),
            },
            "cpu_baseline": cpu,
        }
        print(json.dumps(out), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--config", type=int, default=2, choices=sorted(CONFIGS),
                    help="BASELINE.json config: 2 = beam 5, 4096 reads per GPU (the metric; default), 3 = beam 32, "
                         "8192 reads per GPU (the multi-GPU config's shard), 4 = CRF beam 5, 4096 reads, 5 = the 2-D pair "
                         "consensus on 1024 pairs of 2000 rows (pairs/s)")
    ap.add_argument("--batch", type=int, default=0, help="reads per GPU per step (0 = the config's)")
    ap.add_argument("--cpu-seconds", type=float, default=4.0, help="wall budget of the CPU baseline leg")
    ap.add_argument("--kernel", type=int, default=0,
                    help="0 auto, 1 generic (LDS), 2 wave (two reads/wavefront), 3 wave (one read/wavefront), 4 lane")
    ap.add_argument("--no-viterbi", action="store_true", help="skip the secondary viterbi roofline leg")
    ap.add_argument("--no-e2e", action="store_true", help="skip the host-numpy -> Python objects leg")
    ap.add_argument("--overlap", type=int, default=None,
                    help="fcd_set_overlap (include/fcd.h): successive steps go round-robin to this many INTERNAL streams of "
                         "the one handle and share its one tree arena, so that the stragglers of a step (reads that tie at "
                         "every step) run under the next steps; 0 = every step in stream order.  Default: 4")
    ap.add_argument("--mode", choices=("logsumexp", "max"), default="logsumexp",
                    help="--config 5: LogSpace::add as the reference computes it without its default `fastexp` feature "
                         "(logsumexp: BASELINE.json's north star) or with it (max: what the PyPI wheels compute)")
    ap.add_argument("--streams", type=int, default=1,
                    help="issue successive steps round-robin on this many HIP streams (each with its own "
                         "handle and tree arena) so that independent batches overlap on the GPU; 1 = strictly "
                         "one batch after the other (the default, and what `value` is quoted on)")
    ap.add_argument("--data", choices=("reference", "peaky"), default="reference",
                    help="reference = the metric's generator (tests/test_decode.py:15-17 style rows); "
                         "peaky = softmax rows, a labelled secondary set")
    ap.add_argument("--no-overlap", action="store_true",
                    help="N > 1: run each step's result gather on the compute stream instead of overlapping it "
                         "with the next step's search on a second HIP stream")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise RCCL and run the gather even with one rank (path check on a 1-GPU box)")
    ap.add_argument("--stub", action="store_true",
                    help="TEST ONLY (tests/test_bench_launcher.py): no GPU, no search -- the launcher, the rendezvous "
                         "(gloo), the barriers and the max-over-ranks clock with a sleeping stand-in for the step")
    ap.add_argument("--full", action="store_true",
                    help="also measure what `value` does not need: the CPU baseline and its output check, the e2e leg, "
                         "the rooflines (viterbi included), the tie instrument and the other tie order")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned as DIR/<name>.npy (float32 / float64)")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` by itself: become the launcher of N ranks (one per GPU) of this very script
        raise SystemExit(self_launch(args))
    if args.stub:
        return stub_main(args)
    cfg = CONFIGS[args.config]
    beam, thr = cfg["beam"], cfg["thr"]

    import torch
    import torch.distributed as dist

    import fast_ctc_decode_amd as fcd

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (the launcher and the flag must agree)" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product has no CPU path")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    distributed = world > 1 or args.force_dist
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", str(rank))
        os.environ.setdefault("WORLD_SIZE", str(world))
        dist.init_process_group(backend="nccl", device_id=dev)

    if cfg.get("duplex"):
        return duplex_main(args, cfg, torch, dist, fcd, world, rank, local_rank, dev, distributed)

    B = args.batch or cfg["batch"]
    default_shape = B == cfg["batch"] and args.data == "reference"
    init_host = init = None
    if cfg["crf"]:
        # (T, S=4, N=5) uniform rows, one-hot initial state
        rng = np.random.default_rng(cfg["seed"] + rank)
        x_host = rng.random((B, T, 4, N), dtype=np.float32)
        init_host = np.zeros((B, 4), np.float32)
        init_host[:, 0] = 1.0
        init = torch.from_numpy(init_host).to(dev)
    else:
        x_host = (make_batch if args.data == "reference" else make_batch_peaky)(cfg["seed"] + rank, B)
    x = torch.from_numpy(x_host).to(dev)  # resident in HBM before the timed region
    torch.cuda.synchronize()

    from fast_ctc_decode_amd import dist as fdist
    from fast_ctc_decode_amd import _native as nat
    counts = [B] * world
    scratch = {}
    n_streams = max(1, args.streams)
    handles = [nat.default_handle(local_rank)] + [nat.Handle(local_rank) for _ in range(n_streams - 1)]
    streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in range(n_streams - 1)]
    overlap = cfg.get("overlap", 0) if args.overlap is None else max(0, args.overlap)
    if n_streams > 1 or overlap < 2:
        overlap = 0
    if overlap:
        handles[0].set_overlap(overlap)
    step_no = [0]
    # The gather of step i (RCCL over xGMI, the out_len-prefixed payload packed on the GPU: ~6 KB per read into
    # rank 0) runs on its own HIP stream and overlaps the search of step i+1.  Sizing the payload reads two
    # small values back to the host, so the host issues it one step LATE -- after the search of step i+1 has
    # been queued -- and never leaves the GPU without work; it only reads step i's result tensors, which every
    # call allocates afresh.  flush() issues the last one; all gathers have completed before the closing synchronize.
    comm_stream = torch.cuda.Stream(dev) if distributed and not args.no_overlap else None
    # (overlapping steps: the gather lags as many steps behind as there are further internal streams, so that the host's
    # read-back of the payload size waits for a search that has very likely finished, not for the one just queued)
    from collections import deque
    pending = deque()
    lag = max(1, overlap - 1) if overlap else 1

    def search(s):
        if cfg["crf"]:
            return fcd.crf_beam_search_batch_raw(x, init, beam, thr, kernel=args.kernel)
        return fcd.beam_search_batch_raw(x, beam, thr, True, kernel=args.kernel, handle=handles[s])

    def gather(prev):
        r, ev, slot = prev
        if slot >= 0:  # (the search sat on an internal stream of the handle: the comm stream waits for that one)
            handles[0].overlap_join_slot(slot, comm_stream.cuda_stream)
        else:
            comm_stream.wait_event(ev)
        with torch.cuda.stream(comm_stream):
            for tns in (r.labels, r.path, r.out_len, r.status):
                tns.record_stream(comm_stream)
            fdist.gather_batch_result(r, counts, dst=0, scratch=scratch)

    def flush(keep=0):
        while len(pending) > keep:
            gather(pending.popleft())

    def step():
        s = step_no[0] % n_streams
        step_no[0] += 1
        with torch.cuda.stream(streams[s]):
            r = search(s)
            if distributed and comm_stream is None:
                if overlap:
                    handles[0].overlap_join()  # (the gather reads what an internal stream writes)
                # ONE gather of the packed results to rank 0 (RCCL over xGMI), on the compute stream
                fdist.gather_batch_result(r, counts, dst=0, scratch=scratch)
        if comm_stream is not None:
            ev = torch.cuda.Event()
            ev.record(streams[s])
            pending.append((r, ev, handles[0].overlap_last_slot() if overlap else -1))
            flush(lag)  # earlier steps' results, while this step's search runs
        return r

    def join():
        if overlap:
            handles[0].overlap_join()  # torch's current stream waits for the internal streams (and the kept tensors go)

    for _ in range(args.warmup):
        r = step()
    flush()
    join()
    torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    torch.cuda.synchronize()
    if args.warmup == 0:
        r = step()
        flush()
        join()
    torch.cuda.synchronize()
    if overlap:
        # the results of overlapping steps stay allocated until they are joined: give torch's caching allocator the K sets
        # of result tensors now, so that the timed region does not call hipMalloc
        prime = [[torch.empty_like(t) for t in (r.labels, r.path, r.out_len, r.status) if t is not None]
                 for _ in range(args.steps + 1)]
        del prime
        torch.cuda.synchronize()
    for hh in handles:
        hh.timing_reset()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        r = step()
    flush()  # K searches and K gathers inside the timed region
    join()
    torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    my_elapsed = elapsed

    # kernel duration: the C ABI brackets every launch of the timed region with a HIP event pair
    # on the launch stream (torch's current stream); read them back after the final sync.
    tm = [hh.timing_mean_ms() for hh in handles]
    k_calls = sum(n for _, n in tm)
    k_ms = sum(ms * n for ms, n in tm) / max(k_calls, 1)

    # overlapping steps share the chip, so a launch's own duration above is longer than a launch alone: time that too
    single_ms = None
    if overlap and args.full:
        handles[0].set_overlap(0)
        handles[0].timing_reset()
        for _ in range(min(args.steps, 4)):
            search(0)
        torch.cuda.synchronize()
        single_ms = handles[0].timing_mean_ms()[0]

    t_max = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    per_rank = [None]
    if distributed:
        dist.all_reduce(t_max, op=dist.ReduceOp.MAX)
        # every rank's own clock and search-kernel time, for the record (rank 0 prints them)
        mine = torch.tensor([my_elapsed / args.steps * 1e3, k_ms], dtype=torch.float64, device=dev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank[0] = [[float(v) for v in t.cpu()] for t in allr]
    elapsed = float(t_max.item())

    if rank == 0:
        rc = r.cpu()
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, rc)
        ok = int((rc.status == 0).sum())
        mean_L = float(rc.out_len.astype(np.float64).mean())
        cpu = e2e = vit = vit16 = ties = other_order = roofline = None  # (measured with --full only)
        if args.full:
            # posteriors in, u8 label + u32 time out (CRF: the dense T*S*N figure)
            bytes_per_read = T * N * 4 * (4 if cfg["crf"] else 1) + 5.0 * mean_L
            # Overlapping steps (fcd_set_overlap): `k_ms` is a launch's duration WHILE it shares the chip with the launches of the
            # other internal streams -- on average k_ms * steps / elapsed of them at once -- so the kernel's rate is a launch's
            # bytes over its share of that time, k_ms / launches_in_flight = elapsed / steps.  One launch at a time: k_ms itself.
            in_flight = k_ms * args.steps / (elapsed * 1e3) if overlap else 1.0
            k_eff_ms = k_ms / in_flight if overlap else k_ms
            achieved = B * bytes_per_read / (k_eff_ms * 1e-3) / 1e9
            # the CPU leg (and its output cross-check) runs on rank 0 at N = 1 only, as the contract asks
            cpu = cpu_baseline(cfg, x_host, init_host, rc.labels, rc.path, rc.out_len, args.cpu_seconds) if world == 1 else None
            # (the names carry further template arguments after S: counting / profiling / one-length flags)
            prefix = cfg["kernel_prefix"] if args.kernel == 0 else {
                1: "beam_generic_kernel", 2: "beam_wave_kernel<5, 6, 2, %d" % (4 if cfg["crf"] else 0),
                3: "beam_wave_kernel<5, 8, 1, %d" % (4 if cfg["crf"] else 0), 4: "beam_lane_kernel<5, 2"}[args.kernel]
            traffic, traffic_note = pmc_traffic(prefix) if default_shape else (None, None)
            props = torch.cuda.get_device_properties(dev)
            simds = props.multi_processor_count * 4
            rpw = 1 if args.kernel in (1, 3) else 2
            # outside the timed region: the tie instrument on the same batch (include/fcd.h)
            if cfg["crf"]:
                amb = fcd.crf_beam_search_batch_raw(x, init, beam, thr, count_ambiguous=True).cpu().ambiguous
            else:
                amb = fcd.beam_search_batch_raw(x, beam, thr, True, count_ambiguous=True).cpu().ambiguous
            ties = {"reads_with_gt20_candidate_kept_tie": int((amb[:, 0] > 0).sum()),
                    "reads_with_result_changing_tie": int((amb[:, 1] > 0).sum()),
                    "reads_with_both": int(((amb[:, 0] > 0) & (amb[:, 1] > 0)).sum()),
                    "note": "a read with either counter at 0 decodes the same under any order of equal probabilities; on "
                            "the others the kernels follow the restated order of Rust 1.78's sort_unstable_by "
                            "(FCD_TIE_PDQ178, csrc/pdq178.h; tests/test_gpu_fullsize.py::test_config2_tie_instrument)"}
            # outside the timed region (N = 1): the same launches under the OTHER selectable order of equal probabilities,
            # so that one line from one box shows what the default order (Rust 1.78's) costs against the stable one
            other_order = None
            if world == 1:
                mine_order = fcd.tie_order()
                try:
                    alt = "stable" if mine_order == "pdq178" else "pdq178"
                    fcd.set_tie_order(alt)
                    for _ in range(2):
                        search(0)
                    torch.cuda.synchronize()
                    handles[0].timing_reset()
                    for _ in range(args.steps):
                        search(0)
                    torch.cuda.synchronize()
                    alt_ms, alt_calls = handles[0].timing_mean_ms()
                    other_order = {"tie_order": alt, "kernel_ms": alt_ms, "launches_timed": alt_calls,
                                   "reads_per_s_by_kernel_time": B / (alt_ms * 1e-3),
                                   "this_order_reads_per_s_by_kernel_time": B / ((single_ms or k_ms) * 1e-3)}
                except Exception as e:  # never at the price of the bench line
                    other_order = {"error": str(e)}
                finally:
                    fcd.set_tie_order(mine_order)
            pdq = "1" if fcd.tie_order() == "pdq178" else "0"
            uni = "1"  # (bench batches have one length: the UNI instantiation)
            symbol = {2: "beam_wave_kernelILi5ELi6ELi2ELi0ELb0ELb0ELb%sELb0ELb%sE" % (uni, pdq),
                      3: "beam_lane_kernelILi5ELi2ELb0ELb0ELb%sE" % pdq,
                      4: "beam_wave_kernelILi5ELi6ELi2ELi4ELb0ELb0ELb%sELb0ELb%sE" % (uni, pdq)}.get(args.config)
            occupancy = kernel_occupancy(symbol) if (symbol and args.kernel == 0) else None
            vit = viterbi_roofline(fcd, torch, dev) if not args.no_viterbi else None
            vit16 = viterbi_roofline(fcd, torch, dev, half=True) if not args.no_viterbi else None
            valu = valu_issue_roofline(prefix, k_eff_ms, simds) if default_shape else None
            e2e = None
            if world == 1 and not args.no_e2e and args.streams == 1:
                e2e = e2e_leg(fcd, cfg, x_host, init_host, rc)
            roofline = {
                "bound": "hbm",
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                "traffic": traffic,
                "traffic_source": traffic_note,
                "kernel": "beam search kernel, %.3f ms per launch (HIP events)%s, %d reads x %.0f "
                          "algorithmic B/read" % (k_ms, " with %.2f launches in flight on average = %.3f ms of the chip per launch"
                                                  % (in_flight, k_eff_ms) if overlap else "", B, bytes_per_read),
                "kernel_ms": k_ms, "launches_timed": k_calls, "launches_in_flight": in_flight,
                # The search is a serial chain of T dependent steps per read: it is bound by instruction
                # issue, not by HBM (SURVEY.md finding 5) -- priced here against the VALU issue peak.
                "secondary_bound": valu if valu is not None else {
                    "bound": "valu_issue", "achieved": None, "peak": simds * 2.4e9 / 2.0,
                    "note": "no SQ counter summary of this kernel / shape on the current kernel sources under profiles/"},
                # --overlap: `kernel_ms` is a launch's duration while it shares the chip with the launches of the other
                # internal streams; what the chip sustains is a launch per `sustained_ms_per_launch`
                "overlap": None if not overlap else {
                    "streams": overlap, "sustained_ms_per_launch": elapsed / args.steps * 1e3,
                    "achieved_one_launch_at_a_time": B * bytes_per_read / (single_ms * 1e-3) / 1e9 if single_ms else None,
                    "single_launch_ms": single_ms,
                    "single_launch_reads_per_s": B / (single_ms * 1e-3) if single_ms else None},
                "wavefronts_per_simd": B / rpw / simds,
                # (what the instantiation RESERVES: registers, LDS and the resident wavefronts per SIMD they allow)
                "occupancy": occupancy,
                "step_latency_us": (single_ms or k_ms) * 1e3 / T,  # (of a launch alone)
            }
        out = {
            "metric": "reads/s (T=4000, N=5, beam=%d)" % beam,
            "value": world * B * args.steps / elapsed,
            "unit": "reads/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "ranks": {"world_size": dist.get_world_size() if distributed else 1, "backend": "rccl" if distributed else None,
                      "per_rank_ms_per_step": [p[0] for p in per_rank[0]] if per_rank[0] else None,
                      "per_rank_search_kernel_ms": [p[1] for p in per_rank[0]] if per_rank[0] else None,
                      # what a step costs beyond its search kernel: the result gather (pack, RCCL, unpack on rank 0)
                      # and launch gaps, on the slowest rank
                      "step_ms_beyond_the_search_kernel": elapsed / args.steps * 1e3 - k_ms},
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": ("crf_beam_search 4 states x 5 symbols beam_size=%d beam_cut_threshold=%.1f, " % (beam, thr)
                             if cfg["crf"] else
                             "beam_search beam_size=%d beam_cut_threshold=%.1f collapse_repeats, " % (beam, thr))
                            + "batch=%d reads T=4000 N=5 per GPU (%s), " % (B, cfg["baseline"])
                            + ("uniform rows, one-hot init, numpy default_rng(%d+rank)" % cfg["seed"] if cfg["crf"]
                               else "reference-style rows numpy default_rng(%d+rank)" % cfg["seed"]
                               if args.data == "reference"
                               else "SECONDARY SET: peaky softmax rows (logits 4*N(0,1)), default_rng(%d+rank)" % cfg["seed"]),
                "baseline_config": args.config,
                "reads_per_gpu": B, "T": T, "N": N, "beam_size": beam, "beam_cut_threshold": thr,
                "parallelism": ("reads sharded x%d, one RCCL gather of results per step%s"
                                % (world, "" if args.no_overlap else " (on a second stream, overlapping the next step)"))
                               if world > 1 else "single GPU",
                "kernel": cfg["kernel_name"] if args.kernel == 0 else
                          {1: "generic-lds", 2: "wave-registers-2reads", 3: "wave-registers-1read", 4: "lane"}[args.kernel],
                "reads_ok": ok, "mean_labels_per_read": mean_L, "streams": n_streams,
                # fcd_set_overlap: steps round-robin on internal streams of ONE handle with ONE tree arena (slab_pool.h)
                "overlap": overlap,
                "tie_instrument": ties,
                "tie_order": fcd.tie_order(),  # include/fcd.h FCD_TIE_*: pdq178 = Rust 1.78's sort_unstable_by (default)
                "other_tie_order": other_order,
            },
            "full": args.full,
            "roofline": roofline,
            "cpu_baseline": cpu,
            "e2e": e2e,
            "viterbi_roofline": vit,
            "viterbi_roofline_f16": vit16,
        }
        try:  # RCCL's start-up banner sits in C stdio's buffer: push it out so that the JSON line comes LAST
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
