"""CPU-only: the register budget of the headline beam_wave_kernel instantiations, read off the gfx950 code object inside
the built libfcd_hip.so (as bench.py's kernel_occupancy does).  512 VGPRs per SIMD lane in granules of 8: at most 96
VGPRs for five resident wavefronts per SIMD, and no scratch -- a spill in the time loop costs more than the fifth
wavefront gives.

Both headline instantiations meet it with the rank's comparands streamed, a six-register row FIFO, the read's index
formed again after the time loop, and -- PDQ -- the loop-carried state parked in LDS around the inlined quicksort of the
rare tie branch: exact rank (FCD_TIE_STABLE) 78 VGPRs, PDQ (the default tie order, the benchmark's headline) 95, no
scratch in either."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
BUDGET_VGPR = 96  # five wavefronts per SIMD

# beam_wave_kernel<N = 5, GW = 6, RPW = 2, S = 0, AMB = 0, PROF = 0, UNI = 1, H16 = 0, PDQ, NB = 0, SES = 0>
HEADLINE = {
    "uni_pdq": "beam_wave_kernelILi5ELi6ELi2ELi0ELb0ELb0ELb1ELb0ELb1ELb0ELb0EE",
    "uni_exact": "beam_wave_kernelILi5ELi6ELi2ELi0ELb0ELb0ELb1ELb0ELb0ELb0ELb0EE",
}


def _tools():
    return [shutil.which("objcopy"), os.path.join(LLVM, "clang-offload-bundler"), os.path.join(LLVM, "llvm-readelf")]


@pytest.fixture(scope="module")
def kernel_notes():
    """The AMDGPU metadata notes of every gfx950 code object in the library that holds a beam_wave_kernel."""
    if not all(t and os.path.exists(t) for t in _tools()):
        pytest.skip("objcopy / the ROCm LLVM tools are not installed")
    from fast_ctc_decode_amd import _native, build
    build.build()
    tmp = tempfile.mkdtemp(prefix="fcd_budget_")
    try:
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", _native.LIB_PATH, tmp + "/fat.bin"])
        blob = open(tmp + "/fat.bin", "rb").read()
        # the section holds one offload bundle per translation unit, back to back
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)] + [len(blob)]
        notes = ""
        for a, b in zip(starts, starts[1:]):
            if b"beam_wave_kernel" not in blob[a:b]:
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
                          for k in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
    return found


@pytest.mark.parametrize("which", sorted(HEADLINE))
def test_headline_instantiation_fits_five_wavefronts_per_simd(kernel_notes, which):
    found = _meta(kernel_notes, HEADLINE[which])
    assert len(found) == 1, "expected exactly one %s in libfcd_hip.so, found %d" % (HEADLINE[which], len(found))
    m = found[0]
    print("%s: vgpr_count %d, scratch %d B, LDS %d B" % (which, m["vgpr_count"], m["private_segment_fixed_size"],
                                                          m["group_segment_fixed_size"]))
    assert m["private_segment_fixed_size"] == 0, "scratch in the time loop: %r" % m
    assert m["vgpr_count"] <= BUDGET_VGPR, "more than %d VGPRs, fewer than five wavefronts per SIMD: %r" % (BUDGET_VGPR, m)
    # 160 KiB of LDS per CU, a workgroup of four wavefronts = one per SIMD: five workgroups must fit
    assert 5 * m["group_segment_fixed_size"] <= 160 * 1024, "LDS admits fewer than five workgroups per CU: %r" % m
