"""CPU-only: crf_greedy_kernel -- which carries crf_greedy_search's walk, the CRF Viterbi walk and the transition-probability
walk (csrc/viterbi.hip) -- read off the gfx950 code object inside the built libfcd_hip.so as tests/test_crf_lattice_budget.py
reads the lattice kernels: no scratch (a spill in the time loop of a one-wavefront walk costs more than any register it
frees) and the 256 VGPRs of a 64-lane workgroup's budget.  Prints the counts."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
KERNEL = "crf_greedy_kernelE"  # (the mangled name's tail: not crf_greedy_stream_kernel)


@pytest.fixture(scope="module")
def kernel_notes():
    tools = [shutil.which("objcopy"), os.path.join(LLVM, "clang-offload-bundler"), os.path.join(LLVM, "llvm-readelf")]
    if not all(t and os.path.exists(t) for t in tools):
        pytest.skip("objcopy / the ROCm LLVM tools are not installed")
    from fast_ctc_decode_amd import _native, build
    build.build()
    tmp = tempfile.mkdtemp(prefix="fcd_tr_budget_")
    try:
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", _native.LIB_PATH, tmp + "/fat.bin"])
        blob = open(tmp + "/fat.bin", "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)] + [len(blob)]
        notes = ""
        for a, b in zip(starts, starts[1:]):
            if b"crf_greedy_kernel" not in blob[a:b]:
                continue
            with open(tmp + "/one.bin", "wb") as f:
                f.write(blob[a:b])
            subprocess.check_call([LLVM + "/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   "--input=" + tmp + "/one.bin", "--output=" + tmp + "/dev.co", "--unbundle"])
            notes += subprocess.check_output([LLVM + "/llvm-readelf", "--notes", tmp + "/dev.co"]).decode()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return notes


def test_crf_greedy_kernel_has_no_scratch(kernel_notes):
    found = []
    for blk in re.split(r"\n\s*- \.agpr_count", kernel_notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name and KERNEL in name.group(1):
            found.append({k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                          for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "kernarg_segment_size")})
    assert len(found) == 1, "expected exactly one crf_greedy_kernel in libfcd_hip.so, found %d" % len(found)
    m = found[0]
    print("crf_greedy_kernel: vgpr_count %d, sgpr_count %d, scratch %d B, kernel arguments %d B"
          % (m["vgpr_count"], m["sgpr_count"], m["private_segment_fixed_size"], m["kernarg_segment_size"]))
    assert m["private_segment_fixed_size"] == 0, "scratch in the time loop: %r" % m
    assert m["vgpr_count"] <= 256, m
    # the transition-probability walk is in there: its description rides in the kernel's arguments
    assert m["kernarg_segment_size"] >= 240, m
