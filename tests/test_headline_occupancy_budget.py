"""CPU-only: what the headline family of beam_wave_kernel (two reads per wavefront, reads of one length; S = 0 and the
CRF twin S = 4; default tie order and exact rank) takes of a SIMD, read off the resource notes of the gfx950 code object
inside the built libfcd_hip.so, the way tests/test_wave_kernel_budget.py does.  Six wavefronts per SIMD: at most 80 VGPRs
(512 per SIMD lane in granules of 8), no scratch, and at most 27 264 B of LDS per workgroup of four wavefronts (160 KiB
per CU: six workgroups).  Figures reached: exact rank 70 (S = 0) and 76 (S = 4) VGPRs, 3 584 B; default order 80 VGPRs,
22 528 B; no scratch in any."""
import pytest

from test_wave_kernel_budget import _meta, kernel_notes  # noqa: F401  (the fixture)

WAVES = 6
BUDGET_VGPR = 80
BUDGET_LDS = 27264

# beam_wave_kernel<N = 5, GW = 6, RPW = 2, S, AMB = 0, PROF = 0, UNI = 1, H16 = 0, PDQ, NB = 0, SES = 0>
FAMILY = {
    "uni_pdq": "beam_wave_kernelILi5ELi6ELi2ELi0ELb0ELb0ELb1ELb0ELb1ELb0ELb0EE",
    "uni_exact": "beam_wave_kernelILi5ELi6ELi2ELi0ELb0ELb0ELb1ELb0ELb0ELb0ELb0EE",
    "uni_crf4_pdq": "beam_wave_kernelILi5ELi6ELi2ELi4ELb0ELb0ELb1ELb0ELb1ELb0ELb0EE",
    "uni_crf4_exact": "beam_wave_kernelILi5ELi6ELi2ELi4ELb0ELb0ELb1ELb0ELb0ELb0ELb0EE",
}


@pytest.mark.parametrize("which", sorted(FAMILY))
def test_headline_family_fits_six_wavefronts_per_simd(kernel_notes, which):  # noqa: F811
    found = _meta(kernel_notes, FAMILY[which])
    assert len(found) == 1, "expected exactly one %s in libfcd_hip.so, found %d" % (FAMILY[which], len(found))
    m = found[0]
    print("%s: vgpr_count %d, scratch %d B, LDS %d B" % (which, m["vgpr_count"], m["private_segment_fixed_size"],
                                                          m["group_segment_fixed_size"]))
    assert m["private_segment_fixed_size"] == 0, "scratch: %r" % m
    assert m["vgpr_count"] <= BUDGET_VGPR, "more than %d VGPRs, fewer than %d wavefronts per SIMD: %r" % (BUDGET_VGPR, WAVES, m)
    assert m["group_segment_fixed_size"] <= BUDGET_LDS, "LDS admits fewer than %d workgroups per CU: %r" % (WAVES, m)
    assert WAVES * m["group_segment_fixed_size"] <= 160 * 1024
