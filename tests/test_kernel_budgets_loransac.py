"""The two one-wavefront-per-problem LO-RANSAC kernels (rr_pairs_kernel: its own walk; ap_images_kernel: loransac_walk.h's walk),
checked without a GPU on the cross-compiled gfx950 resource report (flags and parsing of tests/test_kernel_budgets.py).  The limits
are what the kernels used while each estimator had a walk of its own; the rotation kernel's LDS limit is the point at
which six workgroups still fit a CU."""
import pytest

from test_kernel_budgets import HIPCC, compile_device, one

pytestmark = pytest.mark.skipif(not __import__("os").path.exists(HIPCC), reason="hipcc not installed")


def test_rotation_walk_keeps_two_waves_and_six_workgroups(tmp_path_factory):
    _, k = compile_device("relrot", tmp_path_factory)
    r, _ = one(k, "rr_pairs_kernel")
    assert r["VGPRs Spill"] == 0 and r["ScratchSize"] <= 32 and r["Occupancy"] >= 2, r
    assert r["LDS Size"] <= 26624, r  # six workgroups per 160 KB CU


def test_absolute_pose_walk_keeps_its_registers_and_lds(tmp_path_factory):
    _, k = compile_device("abspose", tmp_path_factory)
    r, _ = one(k, "ap_images_kernel")
    assert r["VGPRs Spill"] == 0 and r["AGPRs"] == 0 and r["ScratchSize"] <= 528 and r["LDS Size"] <= 34376, r
