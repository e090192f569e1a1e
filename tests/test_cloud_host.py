"""The point-cloud filters of ``opensfm_amd/csrc/cloud.hip`` without a GPU: the numpy restatements of ``tests/cloud_cases.py`` against a
50-digit evaluation and against the reference's compiled kd-tree, the kernels themselves on the host emulation of HIP
(``tests/native/build_cloud_emu.py``) against the restatements, the reference's own ``remove_outliers`` over
``geometry_types.Reconstruction``, and the two ``pysfm`` names against the reference's binding."""
import contextlib
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import cloud_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/opensfm"
OUT = os.path.join(HERE, "native", "_build")
need_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference is not mounted")


# ---- the restatement against truth ----
@pytest.mark.parametrize("model", cases.MODELS)
def test_conditioning_restatement_against_50_digits(model):
    """cond of the restatement (float64 duals, inv + eigvalsh as the reference) within rtol 1e-8 of the same formulas at 50 digits with
    mpmath-differentiated Jacobians.  A Jacobi / QR eigen-solve of H errs by a few eps * kappa(H) <= 1e-16 * 1e6 relative on the smallest
    eigenvalue before the clamp at 1 000, half of that after the square root: 1e-8 leaves a factor of ~30."""
    scene = cases.model_scene(model)
    res = cases.conditioning_reference("model", model)
    picked = np.flatnonzero(np.isin(res["reason"], (0, 5)))[:10]
    assert len(picked) == 10
    truth = cases.conditioning_truth_mp(scene, picked)
    assert np.isfinite(truth).all() and (truth < cases.MAX_COND).all()
    np.testing.assert_allclose(res["cond"][picked], truth, rtol=1e-8, atol=0)


def test_conditioning_restatement_special_cases_against_50_digits():
    """the street scene: the wide pair, the clamped pair and the first ragged tracks (2 .. 200 observations)"""
    scene = cases.conditioning_scene(65)
    res = cases.conditioning_reference("scene", 65)
    assert list(res["reason"][:7]) == [1, 1, 0, 1, 2, 0, 3] or list(res["reason"][:7]) == [1, 1, 0, 1, 2, 5, 3]
    assert res["cond"][5] == cases.MAX_COND
    picked = [p for p in (2, 5, 8, 9, 10, 11, 12, 15) if res["reason"][p] in (0, 5)]
    assert 5 in picked and len(picked) >= 6
    truth = cases.conditioning_truth_mp(scene, picked)
    np.testing.assert_allclose(res["cond"][picked], truth, rtol=1e-8, atol=0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 3000])
def test_conditioning_scene_has_no_borderline_landmark(n):
    """the seeds of the scenes the GPU tests demand identical removal sets on: no decision of the restatement hangs on rounding"""
    res = cases.conditioning_reference("scene", n)
    assert len(cases.borderline(res)) == 0
    if n >= 63:
        assert set(np.unique(res["reason"])) >= {0, 1, 2, 3, 5}


@pytest.mark.parametrize("model", cases.MODELS)
def test_model_scene_has_no_borderline_landmark(model):
    res = cases.conditioning_reference("model", model)
    assert len(cases.borderline(res)) == 0 and (res["reason"] == 0).sum() >= 30


# ---- isolation against the reference's compiled kd-tree ----
@pytest.fixture(scope="module")
def kdtree():
    vl = os.path.join(REF, "src", "third_party", "vlfeat")
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, "cloud_kdtree_ref.so")
    src = os.path.join(HERE, "native", "cloud_kdtree_adapter.c")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        # as the reference builds vlfeat on x86 (third_party/vlfeat/CMakeLists.txt: SSE2 on, AVX off), no contraction
        flags = ["-O2", "-msse2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=gnu99", "-w", "-DVL_DISABLE_AVX", "-DVL_DISABLE_THREADS",
                 "-DVL_DISABLE_OPENMP", "-I", vl]
        units = [os.path.join(vl, "vl", f) for f in ("kdtree.c", "generic.c", "host.c", "random.c", "mathop.c", "mathop_sse2.c", "mathop_avx.c")]
        subprocess.check_call(["gcc", *flags, "-shared", "-o", so, src, *units, "-lm"])
    lib = C.CDLL(so)
    lib.ref_isolation_averages.restype = C.c_int
    lib.ref_isolation_averages.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_double)]
    return lib


@need_ref
@pytest.mark.parametrize("name", cases.KDTREE_CLOUDS)
def test_isolation_restatement_equals_the_kdtree(kdtree, name):
    pts = np.ascontiguousarray(cases.cloud(name), np.float64)
    avg = np.zeros(len(pts))
    assert kdtree.ref_isolation_averages(pts.ctypes.data_as(C.POINTER(C.c_double)), len(pts), 7, avg.ctypes.data_as(C.POINTER(C.c_double))) == 0
    ref = cases.isolation_reference(name, 7)
    if len(pts) <= 7:
        assert ref["count"] == 0
    else:
        assert np.array_equal(avg, ref["avg"])  # bit-equal


# ---- the kernels on the CPU ----
@contextlib.contextmanager
def emulated_cloud():
    """inside: opensfm_amd calls that go through _lib.load() run cloud.hip on the host emulation"""
    from opensfm_amd import _lib

    spec = importlib.util.spec_from_file_location("build_cloud_emu", os.path.join(HERE, "native", "build_cloud_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = C.CDLL(mod.build())
    for name, (res, args) in _lib._signatures().items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    old_lib, old_ctx = _lib._lib, getattr(_lib._tls, "ctx", None)
    _lib._lib, _lib._tls.ctx = lib, {}
    try:
        yield lib
    finally:
        for c in _lib._tls.ctx.values():
            c.close()
        _lib._lib, _lib._tls.ctx = old_lib, old_ctx


@pytest.fixture(scope="module")
def emu():
    with emulated_cloud() as lib:
        yield lib


def run_conditioning(scene, **kw):
    from opensfm_amd import opensfm_adapter

    return opensfm_adapter.points_conditioning(scene["points"], scene["shot_pose"], scene["shot_camera"], scene["cam_model"], scene["cam_params"],
                                               scene["obs_shot"], scene["obs_point"], **kw)


# (overfull with k = 31 is 16 M insertions into a 32-entry list, minutes on the emulation: the GPU suite runs it)
@pytest.mark.parametrize("name,k", [(name, k) for k in (7, 1, 31) for name in cases.CLOUDS if (name, k) != ("overfull", 31)])
def test_emulated_isolation_is_bit_equal(emu, name, k):
    from opensfm_amd import opensfm_adapter

    cases.check_isolation(opensfm_adapter.points_isolation(cases.cloud(name), k), cases.isolation_reference(name, k))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_emulated_conditioning_scene(emu, n):
    cases.check_conditioning(run_conditioning(cases.conditioning_scene(n)), cases.conditioning_reference("scene", n))


@pytest.mark.parametrize("model", cases.MODELS)
def test_emulated_conditioning_models(emu, model):
    cases.check_conditioning(run_conditioning(cases.model_scene(model)), cases.conditioning_reference("model", model))


def test_emulated_edge_cases(emu):
    from opensfm_amd import _lib, opensfm_adapter

    launches = emu.hipemu_launch_count
    launches.restype = C.c_long
    before = launches()
    empty = opensfm_adapter.points_isolation(np.zeros((0, 3)))
    assert empty["count"] == 0 and len(empty["avg"]) == 0
    scene = cases.conditioning_scene(65)
    none = opensfm_adapter.points_conditioning(np.zeros((0, 3)), scene["shot_pose"], scene["shot_camera"], scene["cam_model"], scene["cam_params"],
                                               np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert none["removed"] == 0 and np.isnan(none["threshold"])
    no_obs = opensfm_adapter.points_conditioning(scene["points"], scene["shot_pose"], scene["shot_camera"], scene["cam_model"], scene["cam_params"],
                                                 np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert (no_obs["reason"] == 1).all() and no_obs["removed"] == 65
    assert launches() == before  # n_points == 0 and n_obs == 0: no launch
    for k in (0, 32):
        with pytest.raises(_lib.OsfmError, match=r"\(-1\)"):
            opensfm_adapter.points_isolation(cases.cloud("n9"), k)
    bad = np.array(cases.cloud("uniform"))
    bad[17, 1] = np.nan
    with pytest.raises(_lib.OsfmError, match=r"\(-1\)"):
        opensfm_adapter.points_isolation(bad)
    bad[17, 1] = 1e300  # infinite as a float32
    with pytest.raises(_lib.OsfmError, match=r"\(-1\)"):
        opensfm_adapter.points_isolation(bad)
    with pytest.raises(_lib.OsfmError, match=r"\(-1\)"):
        run_conditioning(dict(scene, obs_point=scene["obs_point"] + 1000))
    shot_camera = np.array(scene["shot_camera"])
    shot_camera[2] = len(scene["cam_model"])
    with pytest.raises(_lib.OsfmError, match=re.escape("(-1): osfm_points_conditioning: shot 2 names a camera outside the table") + "$"):
        run_conditioning(dict(scene, shot_camera=shot_camera))
    cam_model = np.array(scene["cam_model"])
    cam_model[0] = 99
    with pytest.raises(_lib.OsfmError, match=re.escape("(-1): osfm_points_conditioning: camera 0 has model 99") + "$"):
        run_conditioning(dict(scene, cam_model=cam_model))


def test_far_points_reach_the_brute_force_kernel(emu):
    """gaussian_far is the cloud that covers knn_brute_kernel and its 64-lane merge: its far points must stay open after the ring budget,
    which shows as a second launch.  A change of the grid heuristics that routes every query through the rings fails here instead of
    silently losing that coverage.  The uniform cloud is settled by the rings alone."""
    from opensfm_amd import opensfm_adapter

    launches = emu.hipemu_launch_count
    launches.restype = C.c_long
    for k in (1, 7, 31):
        before = launches()
        opensfm_adapter.points_isolation(cases.cloud("gaussian_far"), k)
        assert launches() - before == 2
    before = launches()
    opensfm_adapter.points_isolation(cases.cloud("uniform"), 7)
    assert launches() - before == 1


def test_emulated_python_filters_remove_what_the_restatement_removes(emu):
    """compat.pysfm on a reconstruction with rigs and two camera models"""
    cases.check_python_filters()


# ---- remove_outliers of the reference's own file over geometry_types.Reconstruction ----
def planted_reconstruction():
    r = cases.bundle_reconstruction()
    rng = np.random.default_rng(1)
    for lm_id, lm in r.points.items():
        for shot_id, shot in r.shots.items():
            if lm_id in shot.observations:
                lm.reprojection_errors[shot_id] = rng.normal(0, 5e-4, 2)
    with_many = [lm for lm in r.points if r.points[lm].number_of_observations() >= 4]
    with_two = with_many[-3:]  # cut down to two observations each
    for lm_id in with_two:
        for shot_id in list(r.points[lm_id].reprojection_errors)[2:]:
            r.remove_observation(shot_id, lm_id)
            del r.points[lm_id].reprojection_errors[shot_id]
        assert r.points[lm_id].number_of_observations() == 2
    planted = []
    for lm_id in with_many[:6]:  # one gross error each: the landmark stays
        shot_id = next(iter(r.points[lm_id].reprojection_errors))
        r.points[lm_id].reprojection_errors[shot_id] = np.array([0.05, -0.04])
        planted.append((lm_id, shot_id))
    doomed = with_two[:3]  # one of two observations: the landmark goes
    for lm_id in doomed:
        shot_id = next(iter(r.points[lm_id].reprojection_errors))
        r.points[lm_id].reprojection_errors[shot_id] = np.array([-0.03, 0.06])
        planted.append((lm_id, shot_id))
    assert len(doomed) == 3
    return r, planted, doomed


@need_ref
@pytest.mark.parametrize("filtering", ["FIXED", "AUTO"])
def test_reference_remove_outliers_runs_on_the_map(filtering):
    import bundle_cases

    ref = bundle_cases.load_reference_reconstruction()
    r, planted, doomed = planted_reconstruction()
    before = {s: set(shot.observations) for s, shot in r.shots.items()}
    n_points = len(r.points)
    config = {"bundle_outlier_filtering_type": filtering, "bundle_outlier_fixed_threshold": 0.006, "bundle_outlier_auto_ratio": 3.0}
    assert ref.remove_outliers(r, config) == len(planted)
    gone = {(s, lm) for s in before for lm in before[s] - set(r.shots[s].observations)}
    expected = {(s, lm) for lm, s in planted} | {(s, lm) for lm in doomed for s in before if lm in before[s]}
    assert gone == expected
    assert set(doomed).isdisjoint(r.points) and len(r.points) == n_points - len(doomed)
    assert len(r.get_landmarks()) == len(r.points)


def test_own_outlier_step_matches():
    """opensfm_amd.reconstruction.discard_gross_observations (for callers without the reference's module) does the same"""
    from opensfm_amd import reconstruction as gpu_reconstruction

    r, planted, doomed = planted_reconstruction()
    config = {"bundle_outlier_filtering_type": "AUTO", "bundle_outlier_auto_ratio": 3.0}
    before = {s: set(shot.observations) for s, shot in r.shots.items()}
    n_points = len(r.points)
    assert gpu_reconstruction.discard_gross_observations(r, config) == len(planted)
    gone = {(s, lm) for s in before for lm in before[s] - set(r.shots[s].observations)}
    assert gone == {(s, lm) for lm, s in planted} | {(s, lm) for lm in doomed for s in before if lm in before[s]}
    assert set(doomed).isdisjoint(r.points) and len(r.points) == n_points - len(doomed)
    fixed = {"bundle_outlier_filtering_type": "FIXED", "bundle_outlier_fixed_threshold": 0.006}
    r, planted, doomed = planted_reconstruction()
    assert gpu_reconstruction.discard_gross_observations(r, fixed) == len(planted) and set(doomed).isdisjoint(r.points)
    with pytest.raises(KeyError):
        gpu_reconstruction.discard_gross_observations(r, {})


def test_landmark_outside_a_map_has_no_observation_count():
    """a Landmark that Reconstruction.create_point did not make cannot count its observations: an error, not a silent 0 that the
    outlier step would read as 'remove it'"""
    from opensfm_amd.geometry_types import Landmark

    with pytest.raises(RuntimeError):
        Landmark("p0", [0.0, 0.0, 1.0]).number_of_observations()


def test_removing_landmarks_does_not_walk_the_shots():
    """remove_landmark and number_of_observations go through the per-landmark set of observing shots"""
    r = cases.bundle_reconstruction()

    class Forbidden(dict):
        def values(self):
            raise AssertionError("walked every shot")

        items = __iter__ = values

    observers = {lm: {s for s, shot in r.shots.items() if lm in shot.observations} for lm in r.points}
    shots, r.shots = r.shots, Forbidden(r.shots)
    for lm_id in list(r.points)[:20]:
        assert r.points[lm_id].number_of_observations() == len(observers[lm_id])
        r.remove_landmark(r.points[lm_id])
        assert all(lm_id not in shots[s].observations for s in observers[lm_id])


# ---- names and signatures ----
def test_pysfm_names_and_defaults():
    from opensfm_amd.compat import pysfm

    sig = inspect.signature(pysfm.filter_badly_conditioned_points)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [("map", inspect.Parameter.empty), ("min_angle_deg", 1.0), ("min_abs_det", 1e-15)]
    sig = inspect.signature(pysfm.remove_isolated_points)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [("map", inspect.Parameter.empty), ("k", 7)]


@need_ref
def test_pysfm_signatures_against_the_binding():
    from opensfm_amd.compat import pysfm

    text = open(os.path.join(REF, "src", "sfm", "python", "pybind.cc")).read()
    for name in ("filter_badly_conditioned_points", "remove_isolated_points"):
        block = re.search(r'm\.def\("%s",(.*?)\);' % name, text, re.S).group(1)
        declared = [(a, d) for a, d in re.findall(r'py::arg\("(\w+)"\)(?:\s*=\s*([-\w.+]+))?', block)]
        ours = [(p.name, p.default) for p in inspect.signature(getattr(pysfm, name)).parameters.values()]
        assert [a for a, _ in declared] == [a for a, _ in ours]
        for (_, d), (_, default) in zip(declared, ours):
            assert (d == "" and default is inspect.Parameter.empty) or float(d) == float(default)
