"""CPU-only: crf_greedy_kernel with the fourth walk in it -- the marginals' forward pass (csrc/viterbi.hip,
crf_marginals_forward, va.mode == 3) -- read off the gfx950 code object inside the built libfcd_hip.so as
tests/test_crf_transitions_budget.py reads it: still ONE kernel (the forward pass is a walk inside it, not a __global__
function of its own), no scratch, and the register count of the build without the fourth walk: 64 VGPRs, the most a wavefront
may hold with eight wavefronts resident on a SIMD (512 / 64), so that crf_greedy_search's, the Viterbi and the
transition-probability walk lose no wavefront to it.  Prints the counts."""
import re

from test_crf_transitions_budget import KERNEL, kernel_notes  # noqa: F401  (the fixture that unbundles the code object)

PARENT_VGPRS = 64   # crf_greedy_kernel built from the commit before the marginals
OCCUPANCY_STEP = 64  # 512 VGPRs per lane of a SIMD / 8 wavefronts


def _kernels(notes):
    found = []
    for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name and KERNEL in name.group(1):
            found.append({k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                          for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "kernarg_segment_size")})
    return found


def test_one_kernel_no_scratch_and_the_parents_occupancy(kernel_notes):  # noqa: F811
    found = _kernels(kernel_notes)
    assert len(found) == 1, "expected exactly one crf_greedy_kernel in libfcd_hip.so, found %d" % len(found)
    m = found[0]
    print("crf_greedy_kernel: vgpr_count %d (parent %d), sgpr_count %d, scratch %d B, kernel arguments %d B"
          % (m["vgpr_count"], PARENT_VGPRS, m["sgpr_count"], m["private_segment_fixed_size"], m["kernarg_segment_size"]))
    assert m["private_segment_fixed_size"] == 0, "scratch in the time loop: %r" % m
    assert PARENT_VGPRS <= OCCUPANCY_STEP
    assert m["vgpr_count"] <= OCCUPANCY_STEP, "the fourth walk costs the other three a wavefront per SIMD: %r" % m
