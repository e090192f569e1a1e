"""``osfm_points_isolation`` / ``osfm_points_conditioning`` (opensfm_amd/csrc/cloud.hip) on the GPU against the numpy restatements of
``tests/cloud_cases.py`` -- the module that ``tests/test_cloud_host.py`` pins to a 50-digit evaluation and to the reference's kd-tree.

Isolation is bit-equal by construction: float32 distances in the reference's order without contraction, an exact search, the sum and
the statistics in a fixed order.  Conditioning: rtol 1e-8 on cond and the threshold (a Jacobi eigen-solve of H errs by a few
eps * kappa(H) <= 1e-16 * 1e6 on the smallest eigenvalue before the clamp at 1 000, half of that after the square root; 1e-8 leaves a
factor of ~30 and covers the restatement's inverse-then-eigenvalues route), identical reasons -- the scenes have no borderline landmark,
which ``test_cloud_host.py`` checks on the CPU and these tests assert again."""
import numpy as np
import pytest

import cloud_cases as cases
from opensfm_amd import _lib, opensfm_adapter

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", [7, 1, 31])
@pytest.mark.parametrize("name", cases.CLOUDS)
def test_isolation_is_bit_equal_to_the_restatement(gpu_ctx, name, k):
    ref = cases.isolation_reference(name, k)
    got = opensfm_adapter.points_isolation(cases.cloud(name), k, ctx=gpu_ctx)
    if len(cases.cloud(name)) <= k:
        assert ref["count"] == 0 and not got["removed"].any()  # the reference returns before it computes anything
    cases.check_isolation(got, ref)


def test_isolation_two_runs_are_bit_equal(gpu_ctx):
    for name in ("gaussian_far", "lattice"):
        a = opensfm_adapter.points_isolation(cases.cloud(name), 7, ctx=gpu_ctx)
        b = opensfm_adapter.points_isolation(cases.cloud(name), 7, ctx=gpu_ctx)
        assert a["avg"].tobytes() == b["avg"].tobytes() and a["removed"].tobytes() == b["removed"].tobytes() and a["threshold"] == b["threshold"]


def test_isolation_refuses_bad_arguments(gpu_ctx):
    for k in (0, 32):
        with pytest.raises(_lib.OsfmError, match=r"\(-1\)"):  # OSFM_E_INVALID
            opensfm_adapter.points_isolation(cases.cloud("n9"), k, ctx=gpu_ctx)
    bad = np.array(cases.cloud("uniform"))
    bad[17, 1] = np.nan
    with pytest.raises(_lib.OsfmError, match=r"\(-1\)"):
        opensfm_adapter.points_isolation(bad, ctx=gpu_ctx)
    empty = opensfm_adapter.points_isolation(np.zeros((0, 3)), ctx=gpu_ctx)
    assert empty["count"] == 0 and len(empty["avg"]) == 0


def run_conditioning(scene, ctx):
    return opensfm_adapter.points_conditioning(scene["points"], scene["shot_pose"], scene["shot_camera"], scene["cam_model"], scene["cam_params"],
                                               scene["obs_shot"], scene["obs_point"], ctx=ctx)


def check_conditioning(scene, ref, ctx):
    assert len(cases.borderline(ref)) == 0  # no decision of the restatement hangs on rounding: the removal sets must be identical
    got = run_conditioning(scene, ctx)
    cases.check_conditioning(got, ref)
    again = run_conditioning(scene, ctx)
    assert again["cond"].tobytes() == got["cond"].tobytes() and again["reason"].tobytes() == got["reason"].tobytes()
    assert again["threshold"] == got["threshold"] or (np.isnan(again["threshold"]) and np.isnan(got["threshold"]))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000])
def test_conditioning_special_cases_and_ragged_tracks(gpu_ctx, n):
    """0, 1 and 2 observations, parallel rays, a point at a camera centre, the clamped 1.01 degree pair, the far group under min_abs_det,
    tracks of 2 .. 200 observations across the 8-lane groups"""
    ref = cases.conditioning_reference("scene", n)
    if n >= 63:
        assert list(ref["reason"][:5]) == [1, 1, 0, 1, 2] and ref["cond"][5] == cases.MAX_COND and ref["reason"][6] == 3
    check_conditioning(cases.conditioning_scene(n), ref, gpu_ctx)


@pytest.mark.parametrize("model", cases.MODELS)
def test_conditioning_every_camera_model(gpu_ctx, model):
    check_conditioning(cases.model_scene(model), cases.conditioning_reference("model", model), gpu_ctx)


def test_conditioning_without_points_or_observations(gpu_ctx):
    scene = cases.conditioning_scene(65)
    none = opensfm_adapter.points_conditioning(np.zeros((0, 3)), scene["shot_pose"], scene["shot_camera"], scene["cam_model"], scene["cam_params"],
                                               np.zeros(0, np.int32), np.zeros(0, np.int32), ctx=gpu_ctx)
    assert none["removed"] == 0 and np.isnan(none["threshold"])
    no_obs = opensfm_adapter.points_conditioning(scene["points"], scene["shot_pose"], scene["shot_camera"], scene["cam_model"], scene["cam_params"],
                                                 np.zeros(0, np.int32), np.zeros(0, np.int32), ctx=gpu_ctx)
    assert (no_obs["reason"] == 1).all() and no_obs["removed"] == 65


def test_pysfm_filters_on_a_reconstruction_with_rigs(gpu_ctx):
    """compat.pysfm.filter_badly_conditioned_points / remove_isolated_points and cull_final_point_cloud on a make_bundle_scene
    reconstruction with rigs and two camera models: the map keeps exactly what the restatement keeps"""
    cases.check_python_filters()
