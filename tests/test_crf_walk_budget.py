"""CPU-only: the four one-wavefront-per-read CRF kernels -- crf_greedy_kernel (csrc/viterbi.hip), crf_viterbi_kernel
(csrc/crf_viterbi.hip), crf_transitions_kernel and crf_marginals_kernel (csrc/crf_transitions.hip) -- read off the gfx950
code objects inside the built libfcd_hip.so as tests/test_crf_lattice_budget.py reads the lattice kernels.  Each is there
exactly once and has no scratch (a spill in the time loop of a one-wavefront walk costs more than any register it frees).
The three walks over all labellings keep the 64 VGPRs they had while they shared one kernel, the most a wavefront may hold
with eight wavefronts resident on a SIMD (512 / 64); crf_greedy_search's serial walk keeps the 20 VGPRs and 76 SGPRs it had before
they moved in (profiles/r10a_isa_table.txt), eight wavefronts per SIMD.  Prints the counts."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
WALK_VGPRS = 64
CAPS = {  # kernel -> (vgpr_count, sgpr_count) it may not exceed; None: no cap of its own
    "crf_greedy_kernel": (20, 76),
    "crf_viterbi_kernel": (WALK_VGPRS, None),
    "crf_transitions_kernel": (WALK_VGPRS, None),
    "crf_marginals_kernel": (WALK_VGPRS, None),
}
FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "kernarg_segment_size")


@pytest.fixture(scope="module")
def kernel_notes():
    tools = [shutil.which("objcopy"), os.path.join(LLVM, "clang-offload-bundler"), os.path.join(LLVM, "llvm-readelf")]
    if not all(t and os.path.exists(t) for t in tools):
        pytest.skip("objcopy / the ROCm LLVM tools are not installed")
    from fast_ctc_decode_amd import _native, build
    build.build()
    tmp = tempfile.mkdtemp(prefix="fcd_walk_budget_")
    try:
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", _native.LIB_PATH, tmp + "/fat.bin"])
        blob = open(tmp + "/fat.bin", "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)] + [len(blob)]
        notes = ""
        for a, b in zip(starts, starts[1:]):
            if not any(k.encode() in blob[a:b] for k in CAPS):
                continue
            with open(tmp + "/one.bin", "wb") as f:
                f.write(blob[a:b])
            subprocess.check_call([LLVM + "/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   "--input=" + tmp + "/one.bin", "--output=" + tmp + "/dev.co", "--unbundle"])
            notes += subprocess.check_output([LLVM + "/llvm-readelf", "--notes", tmp + "/dev.co"]).decode()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return notes


def test_each_kernel_once_without_scratch_within_its_registers(kernel_notes):
    found = {k: [] for k in CAPS}
    for blk in re.split(r"\n\s*- \.agpr_count", kernel_notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        for k in CAPS:
            # (the mangled name's own length prefix: `17crf_greedy_kernelE` is not crf_greedy_stream_kernel)
            if name and "%d%sE" % (len(k), k) in name.group(1):
                found[k].append({f: int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1)) for f in FIELDS})
    for k, ms in found.items():
        for m in ms:
            print("%s: vgpr_count %d, sgpr_count %d, scratch %d B, kernel arguments %d B"
                  % (k, m["vgpr_count"], m["sgpr_count"], m["private_segment_fixed_size"], m["kernarg_segment_size"]))
    for k, (vgprs, sgprs) in CAPS.items():
        assert len(found[k]) == 1, "expected exactly one %s in libfcd_hip.so, found %d" % (k, len(found[k]))
        m = found[k][0]
        assert m["private_segment_fixed_size"] == 0, "scratch in the time loop of %s: %r" % (k, m)
        assert m["vgpr_count"] <= vgprs, (k, m)
        assert sgprs is None or m["sgpr_count"] <= sgprs, (k, m)
