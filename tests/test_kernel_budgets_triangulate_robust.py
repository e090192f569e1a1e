"""Resource budgets of the robust triangulation kernels of ``opensfm_amd/csrc/triangulate.hip``, read from the compiler's
kernel-resource-usage remarks of a gfx950 compile (no GPU): no VGPR spill, LDS no larger than the FULL counterpart's plus the mask words,
and the figures DESIGN.md 4d4 records as the limits."""
import pytest

import test_kernel_budgets as budgets

pytestmark = budgets.pytestmark

MASK_WORD_BYTES = 64 * 4  # tri_wave_robust_kernel: one 32-bit mask word per lane in LDS; the group kernel keeps its word in a register
# DESIGN.md 4d4, from this compile: (kernel, rows) -> (VGPRs, scratch bytes per lane, waves per SIMD); no kernel may need more
LIMITS = {("tri_group_robust_kernel", "BearingRows"): (234, 0, 2), ("tri_wave_robust_kernel", "BearingRows"): (215, 176, 2),
          ("tri_group_robust_kernel", "PixelRows"): (235, 32, 2), ("tri_wave_robust_kernel", "PixelRows"): (255, 320, 1)}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return budgets.compile_device("triangulate", tmp_path_factory)[1]


@pytest.mark.parametrize("kernel,rows", sorted(LIMITS))
def test_robust_kernel_budget(kernels, kernel, rows):
    robust, name = budgets.one(kernels, kernel, rows)
    full, _ = budgets.one(kernels, kernel.replace("_robust", "") + "I", rows)
    print(name, robust)
    assert robust["VGPRs Spill"] == 0
    words = MASK_WORD_BYTES if "wave" in kernel else 0
    assert robust["LDS Size"] <= full["LDS Size"] + words
    vgprs, scratch, occupancy = LIMITS[(kernel, rows)]
    assert robust["VGPRs"] <= vgprs and robust["ScratchSize"] <= scratch and robust["Occupancy"] >= occupancy
