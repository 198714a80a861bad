"""CPU-only: every instantiation of the CRF posterior kernels (csrc/crf_posterior.hip) -- the forward pass at 1, 2, 3, 4, 8
states per lane (3: only the deeper tiers use it), the backward pass on its (states per lane, chain slots, labels) tiers --
read off the gfx950 code object inside the built libfcd_hip.so as tests/test_crf_lattice_budget.py reads its kernels, from
the metadata notes only: each appears once, has no scratch -- a spill in the time loop of a latency-bound single-wavefront
kernel costs more than any register it frees -- and stays within the 256 VGPRs of two wavefronts per SIMD."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
# crfp_back_kernel<K, MM, NB>: m nb <= 8 up to 8 states per lane (4 at eight labels), m nb <= 24 up to 3
TIERS = [(k, mm, nb) for mm, nb in ((2, 4), (4, 2)) for k in (1, 2, 4, 8)] + [(k, 1, 8) for k in (1, 2, 4)] + \
        [(k, mm, nb) for mm, nb in ((3, 8), (6, 4)) for k in (1, 2, 3)]
KERNELS = {"back_k%d_m%d_n%d" % t: "crfp_back_kernelILi%dELi%dELi%dEE" % t for t in TIERS}
KERNELS.update({"fwd_k%d" % k: "crfp_fwd_kernelILi%dEE" % k for k in (1, 2, 3, 4, 8)})


@pytest.fixture(scope="module")
def kernel_notes():
    tools = [shutil.which("objcopy"), os.path.join(LLVM, "clang-offload-bundler"), os.path.join(LLVM, "llvm-readelf")]
    if not all(t and os.path.exists(t) for t in tools):
        pytest.skip("objcopy / the ROCm LLVM tools are not installed")
    from fast_ctc_decode_amd import _native, build
    build.build()
    tmp = tempfile.mkdtemp(prefix="fcd_crf_post_budget_")
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
                          for k in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
    return found


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_instantiation_has_no_scratch(kernel_notes, which):
    found = _meta(kernel_notes, KERNELS[which])
    assert len(found) == 1, "expected exactly one %s in libfcd_hip.so, found %d" % (KERNELS[which], len(found))
    m = found[0]
    print("%s: vgpr_count %d, scratch %d B" % (which, m["vgpr_count"], m["private_segment_fixed_size"]))
    assert m["private_segment_fixed_size"] == 0, "scratch in the time loop: %r" % m
    assert m["vgpr_count"] <= 256, m


def test_no_other_instantiation(kernel_notes):
    names = set(re.findall(r"\.name:\s+\S*(crfp_(?:back|fwd)_kernelI\w+?EE)Ev", kernel_notes))
    assert names == set(KERNELS.values()), names ^ set(KERNELS.values())
