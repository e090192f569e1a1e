"""The three kernels of the plane-based two-view solve (plane.hip), checked without a GPU on the cross-compiled gfx950 resource report
(flags and parsing of tests/test_kernel_budgets.py).  pl_motion_kernel and pl_decide_kernel stream over rows and need no scratch.
pl_ransac_kernel spills: every lane of a block of speculative iterations runs a 4-point DLT, whose 9 x 9 Jacobi eigen-solve keeps the
matrix and its eigenvectors (162 doubles, 324 registers) live in one lane; the limits are that compile's figures, which
no change may exceed."""
import pytest

from test_kernel_budgets import HIPCC, compile_device, one

pytestmark = pytest.mark.skipif(not __import__("os").path.exists(HIPCC), reason="hipcc not installed")


def test_ransac_kernel_fits_the_lds_and_its_spill_does_not_grow(tmp_path_factory):
    _, k = compile_device("plane", tmp_path_factory)
    r, _ = one(k, "pl_ransac_kernel")
    assert r["LDS Size"] <= 64 * 1024, r
    assert r["VGPRs Spill"] <= 438 and r["ScratchSize"] <= 1412 and r["LDS Size"] <= 27952, r


def test_motion_and_decide_kernels_need_no_scratch(tmp_path_factory):
    _, k = compile_device("plane", tmp_path_factory)
    for name in ("pl_motion_kernel", "pl_decide_kernel"):
        r, _ = one(k, name)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["LDS Size"] == 0, (name, r)
    assert one(k, "pl_motion_kernel")[0]["Occupancy"] >= 4
