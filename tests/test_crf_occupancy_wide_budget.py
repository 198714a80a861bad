"""CPU-only: the two instantiations that host the LDS-resident CRF walks of fcd_set_crf_lattice_wide -- crfp_fwd_kernel<8>
(crf_forward_walk_lds, sum and store) and crfp_back_kernel<8, 2, 4> (crfp_occ_walk_lds) -- read off the gfx950 code object
inside the built libfcd_hip.so as tests/test_crf_posterior_budget.py reads its kernels: each appears once, uses no scratch
and stays within the 256 VGPRs of two wavefronts per SIMD, with the new loop bodies inside.  That they are inside is what the
library's own symbol says: a build without fcd_set_crf_lattice_wide has nothing to budget."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
HOSTS = {"fwd_k8": "crfp_fwd_kernelILi8EE", "back_k8_m2_n4": "crfp_back_kernelILi8ELi2ELi4EE"}


@pytest.fixture(scope="module")
def kernel_notes():
    tools = [shutil.which("objcopy"), os.path.join(LLVM, "clang-offload-bundler"), os.path.join(LLVM, "llvm-readelf")]
    if not all(t and os.path.exists(t) for t in tools):
        pytest.skip("objcopy / the ROCm LLVM tools are not installed")
    from fast_ctc_decode_amd import _native, build
    build.build()
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "fcd_set_crf_lattice_wide"), "the library has no wide CRF walks"
    tmp = tempfile.mkdtemp(prefix="fcd_crf_wide_budget_")
    try:
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", _native.LIB_PATH, tmp + "/fat.bin"])
        blob = open(tmp + "/fat.bin", "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)] + [len(blob)]
        notes = ""
        for a, b in zip(starts, starts[1:]):
            if b"crfp_back_kernel" not in blob[a:b]:
                continue
            with open(tmp + "/one.bin", "wb") as f:
                f.write(blob[a:b])
            subprocess.check_call([LLVM + "/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   "--input=" + tmp + "/one.bin", "--output=" + tmp + "/dev.co", "--unbundle"])
            notes += subprocess.check_output([LLVM + "/llvm-readelf", "--notes", tmp + "/dev.co"]).decode()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return notes


def _meta(notes, mangled):
    found = []
    for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name and mangled in name.group(1):
            found.append({k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                          for k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")})
    return found


@pytest.mark.parametrize("which", sorted(HOSTS))
def test_hosting_instantiation_once_no_scratch_256_vgprs(kernel_notes, which):
    found = _meta(kernel_notes, HOSTS[which])
    assert len(found) == 1, "expected exactly one %s in libfcd_hip.so, found %d" % (HOSTS[which], len(found))
    m = found[0]
    print("%s: vgpr_count %d, sgpr_count %d, sgpr spills %d, vgpr spills %d, scratch %d B"
          % (which, m["vgpr_count"], m["sgpr_count"], m["sgpr_spill_count"], m["vgpr_spill_count"], m["private_segment_fixed_size"]))
    assert m["private_segment_fixed_size"] == 0, "scratch in the time loop: %r" % m
    assert m["vgpr_count"] <= 256, m
