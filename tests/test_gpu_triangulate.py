"""``osfm_triangulate_bearings`` / ``osfm_triangulate_tracks`` (opensfm_amd/csrc/triangulate.hip) on the GPU against the step-by-step
restatement of ``tests/triangulate_cases.py`` -- the module that ``tests/test_triangulate_host.py`` pins to exact rays and to a 50-digit
minimiser -- with the tolerance measured there: identical statuses and iteration counts (no scene has a borderline comparison, asserted
again here), points within POINT_RTOL."""
import numpy as np
import pytest

import test_triangulate_host as host
import triangulate_cases as cases
from opensfm_amd import _lib, reconstruction

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,arg", cases.ALL_SCENES)
def test_scene_equals_the_restatement_and_two_runs_are_bit_equal(gpu_ctx, kind, arg):
    scene, ref = cases.scene(kind, arg), cases.reference(kind, arg)
    assert cases.borderline(ref) == []
    rays = cases.run_bearings(scene, gpu_ctx)
    cases.check(rays, ref)
    runs = [(cases.run_bearings, rays)]
    if "obs_xy" in scene:
        pixels = cases.run_tracks(scene, gpu_ctx)
        cases.check(pixels, ref)
        runs.append((cases.run_tracks, pixels))
        # the device's bearings against the host-computed ones fed to the other entry point
        assert np.array_equal(pixels[1], rays[1]) and np.array_equal(pixels[2], rays[2])
        assert cases.relative_difference(pixels[0], rays[0]) <= cases.POINT_RTOL
    for run, first in runs:
        again = run(scene, gpu_ctx)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], first[:3]))


def test_exact_rays_give_the_ground_truth(gpu_ctx):
    scene = cases.scene("rays", 0.0)
    assert cases.relative_difference(cases.run_bearings(scene, gpu_ctx)[0], scene["truth"]) <= 1e-12


def test_special_cases(gpu_ctx):
    assert list(cases.run_bearings(cases.scene("special"), gpu_ctx)[1]) == cases.SPECIAL_STATUS
    points, status, _, _ = cases.run_tracks(cases.scene("ref_spherical"), gpu_ctx)
    assert status[0] == 0 and np.allclose(points[0], [0, 0, 1.3763819204711])
    assert cases.run_tracks(cases.scene("ref_coincident"), gpu_ctx)[1][0] == 4
    o = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    points, status, _, _ = reconstruction.triangulate_bearings_arrays(o, np.array([[0.0, 0, 1.0]] * 3), [0, 3], min_angle_deg=0.0, ctx=gpu_ctx)
    assert status[0] == 5 and np.isnan(points[0]).all()


def test_python_dropins_on_a_reconstruction_with_rigs(gpu_ctx):
    host.check_python_dropins()


def test_pygeometry_leaves(gpu_ctx):
    host.check_pygeometry_leaves()


def test_empty_input_and_bad_arguments(gpu_ctx):
    points, status, iterations, ms = reconstruction.triangulate_bearings_arrays(np.zeros((0, 3)), np.zeros((0, 3)), [0], ctx=gpu_ctx)
    assert len(points) == 0 and len(status) == 0 and len(iterations) == 0 and ms == 0.0
    scene = cases.scene("ragged", 65)
    empty = reconstruction.triangulate_tracks_arrays(scene["shot_pose"], scene["shot_camera"], scene["cam_model"], scene["cam_params"],
                                                     np.zeros(0, np.int32), np.zeros((0, 2)), [0], ctx=gpu_ctx)
    assert len(empty[0]) == 0
    only_empty_tracks = reconstruction.triangulate_bearings_arrays(np.zeros((0, 3)), np.zeros((0, 3)), [0, 0, 0], ctx=gpu_ctx)
    assert list(only_empty_tracks[1]) == [1, 1] and np.isnan(only_empty_tracks[0]).all()
    rays = cases.scene("special")
    o, w, off = rays["centers"], rays["bearings"], rays["offsets"]
    invalid = r"\(-1\)"  # OSFM_E_INVALID
    with pytest.raises(_lib.OsfmError, match=invalid):
        reconstruction.triangulate_bearings_arrays(o, w, off, refinement_iterations=-1, ctx=gpu_ctx)
    with pytest.raises(_lib.OsfmError, match=invalid):
        reconstruction.triangulate_bearings_arrays(o, w, off, min_angle_deg=181.0, ctx=gpu_ctx)
    bad = off.copy()
    bad[2], bad[3] = bad[3], bad[2]
    with pytest.raises(_lib.OsfmError, match=invalid):
        reconstruction.triangulate_bearings_arrays(o, w, bad, ctx=gpu_ctx)

    def tracks(**changes):
        s = dict(scene, **changes)
        return reconstruction.triangulate_tracks_arrays(s["shot_pose"], s["shot_camera"], s["cam_model"], s["cam_params"], s["obs_shot"], s["obs_xy"],
                                                        s["offsets"], ctx=gpu_ctx)

    obs_shot = scene["obs_shot"].copy()
    obs_shot[40] = len(scene["shot_pose"])  # the kernel must refuse it without reading the pose table there
    with pytest.raises(_lib.OsfmError, match=invalid):
        tracks(obs_shot=obs_shot)
    obs_xy = scene["obs_xy"].copy()
    obs_xy[5, 0] = np.nan
    with pytest.raises(_lib.OsfmError, match=invalid):
        tracks(obs_xy=obs_xy)
    shot_pose = scene["shot_pose"].copy()
    shot_pose[scene["obs_shot"][-1], 4] = np.inf
    with pytest.raises(_lib.OsfmError, match=invalid):
        tracks(shot_pose=shot_pose)
    shot_camera = scene["shot_camera"].copy()
    shot_camera[0] = -1
    with pytest.raises(_lib.OsfmError, match=invalid):
        tracks(shot_camera=shot_camera)
    cases.check(tracks(), cases.reference("ragged", 65))  # the context still works after the refusals
