"""``osfm_triangulate_bearings_robust`` / ``osfm_triangulate_tracks_robust`` (opensfm_amd/csrc/triangulate.hip) on the GPU against the
step-by-step restatement of ``tests/triangulate_robust_cases.py`` -- the module that ``tests/test_triangulate_robust_host.py`` pins to the
reference's own code -- with the tolerance measured there: identical status, inlier mask, inlier count and tries (no scene has a
borderline comparison, asserted again here), points within POINT_RTOL.  Reads nothing outside the repository."""
import numpy as np
import pytest

import test_triangulate_robust_host as host
import triangulate_cases as full_cases
import triangulate_robust_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,how", cases.ALL_RUNS)
def test_scene_equals_the_restatement_and_two_runs_are_byte_equal(gpu_ctx, kind, how):
    scene, ref = cases.scene(kind), cases.reference(kind, how)
    assert ref["borderline"] == []
    rays = cases.run("bearings", kind, how, gpu_ctx)
    cases.check(rays, ref)
    runs = [("bearings", rays)]
    if "obs_xy" in scene:
        pixels = cases.run("tracks", kind, how, gpu_ctx)
        cases.check(pixels, ref)
        runs.append(("tracks", pixels))
        # the device's bearings against the host-computed ones fed to the other entry point: the same masks
        assert all(np.array_equal(a, b) for a, b in zip(pixels[1:5], rays[1:5]))
        assert full_cases.relative_difference(pixels[0], rays[0]) <= cases.POINT_RTOL
    for entry, first in runs:
        again = cases.run(entry, kind, how, gpu_ctx)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:5], first[:5]))


def test_seeded_run_equals_the_same_draws_given(gpu_ctx):
    seeded = cases.run("bearings", "rays", "seeded", gpu_ctx)
    given = cases.run_bearings(cases.scene("rays"), draws=cases.draws_of("rays", "seeded"), ctx=gpu_ctx)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(seeded[:5], given[:5]))


def test_python_dropins_on_a_reconstruction_with_rigs(gpu_ctx):
    host.check_python_dropins()


def test_empty_input_and_bad_arguments(gpu_ctx):
    host.check_edge_cases(gpu_ctx)
