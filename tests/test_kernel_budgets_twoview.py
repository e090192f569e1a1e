"""The two kernels of the two-view finish (twoview.hip), checked without a GPU on the cross-compiled gfx950 resource report (flags and
parsing of tests/test_kernel_budgets.py).  tv_config_kernel has the shape of rp_finish_kernel: two wavefronts per SIMD, RefineShared
in LDS.  It spills, as its model does -- the LM driver's state around each trial evaluation of refine_relative_pose; the
limits are that compile's figures, which no change may exceed."""
import pytest

from test_kernel_budgets import HIPCC, compile_device, one

pytestmark = pytest.mark.skipif(not __import__("os").path.exists(HIPCC), reason="hipcc not installed")


def test_config_kernel_keeps_two_waves_and_its_spill_does_not_grow(tmp_path_factory):
    _, k = compile_device("twoview", tmp_path_factory)
    r, _ = one(k, "tv_config_kernel")
    assert r["Occupancy"] >= 2 and r["VGPRs Spill"] <= 87 and r["ScratchSize"] <= 496 and r["LDS Size"] <= 7144, r
    finish, _ = one(compile_device("relpose", tmp_path_factory)[1], "rp_finish_kernel")
    assert r["VGPRs Spill"] <= finish["VGPRs Spill"] and r["ScratchSize"] <= finish["ScratchSize"], (r, finish)  # no worse than its model


def test_decide_kernel_needs_no_scratch(tmp_path_factory):
    _, k = compile_device("twoview", tmp_path_factory)
    r, _ = one(k, "tv_decide_kernel")
    assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["LDS Size"] == 0, r
