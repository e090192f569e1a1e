"""The track triangulation of ``opensfm_amd/csrc/triangulate.hip`` without a GPU: the kernels on the host emulation of HIP
(``tests/native/build_triangulate_emu.py``) against the step-by-step restatement of ``tests/triangulate_cases.py``, the restatement against
a 50-digit minimiser and against exact rays, the Python drop-ins over ``geometry_types.Reconstruction`` against a per-track loop, and a
stand-alone sanitised program over the ragged scene."""
import contextlib
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import triangulate_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))


def _builder():
    spec = importlib.util.spec_from_file_location("build_triangulate_emu", os.path.join(HERE, "native", "build_triangulate_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@contextlib.contextmanager
def emulated_triangulation():
    """inside: opensfm_amd calls that go through _lib.load() run triangulate.hip on the host emulation"""
    from opensfm_amd import _lib

    lib = C.CDLL(_builder().build())
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
    with emulated_triangulation() as lib:
        yield lib


# ---- the kernels on the CPU against the restatement ----
_RESULTS = {}


def emulated_result(kind, arg, entry):
    """one emulated run per scene and entry point, shared by the tests below (call with the `emu` fixture active)"""
    key = (kind, arg, entry)
    if key not in _RESULTS:
        _RESULTS[key] = (cases.run_tracks if entry == "tracks" else cases.run_bearings)(cases.scene(kind, arg))
    return _RESULTS[key]


@pytest.mark.parametrize("kind,arg", cases.EMULATED_SCENES)
def test_emulated_scene_equals_the_restatement(emu, kind, arg):
    """identical statuses and iteration counts, points within POINT_RTOL, through both entry points; the scene has no borderline test"""
    scene, ref = cases.scene(kind, arg), cases.reference(kind, arg)
    assert cases.borderline(ref) == []
    cases.check(emulated_result(kind, arg, "bearings"), ref)
    if "obs_xy" in scene:
        cases.check(emulated_result(kind, arg, "tracks"), ref)


def test_point_tolerance_is_100_times_the_measured_difference(emu):
    """POINT_RTOL is derived from what this test measures: the largest relative difference over every emulated scene and entry point"""
    worst = 0.0
    for kind, arg in cases.EMULATED_SCENES:
        scene, ref = cases.scene(kind, arg), cases.reference(kind, arg)
        worst = max(worst, cases.relative_difference(emulated_result(kind, arg, "bearings")[0], ref["points"]))
        if "obs_xy" in scene:
            worst = max(worst, cases.relative_difference(emulated_result(kind, arg, "tracks")[0], ref["points"]))
    print("largest relative difference between the emulated kernels and the restatement: %.3g" % worst)
    assert worst <= cases.MEASURED_POINT_DIFFERENCE  # a larger value means the constant has to be measured again
    assert cases.POINT_RTOL == 100 * cases.MEASURED_POINT_DIFFERENCE


def test_every_status_and_boundary_length_is_covered():
    ref = cases.reference("ragged", 65)
    lengths = np.diff(cases.scene("ragged", 65)["offsets"])
    assert set(cases.LENGTHS) <= set(lengths.tolist()) and {16, 17} <= set(lengths.tolist())
    assert list(ref["status"][:2]) == [1, 1] and (ref["status"][2:11] == 0).all()  # lengths 0 and 1; 2 .. 300 triangulate
    assert ref["status"][18] == 3 and ref["status"][19] == 2  # the gross observation, the point 1e12 away
    assert list(cases.reference("special")["status"]) == cases.SPECIAL_STATUS
    assert {0, 1, 2, 3} <= set(cases.reference("ragged", 3000)["status"].tolist())


def test_reference_test_cases():
    """the cases of the reference's test_triangulation.py"""
    ref = cases.reference("ref_spherical")
    assert ref["status"][0] == 0 and np.allclose(ref["points"][0], [0, 0, 1.3763819204711])
    assert cases.reference("ref_coincident")["status"][0] == 4  # fails on depth, not on angle
    ref = cases.reference("ref_midpoint")
    assert list(ref["status"]) == [0, 4] and np.allclose(ref["points"][0], [0, 0, 1.0])


# ---- the restatement against truth ----
def test_exact_rays_give_the_ground_truth(emu):
    scene, ref = cases.scene("rays", 0.0), cases.reference("rays", 0.0)
    assert (ref["status"] == 0).all()
    assert cases.relative_difference(ref["points"], scene["truth"]) <= 1e-12
    assert cases.relative_difference(cases.run_bearings(scene)[0], scene["truth"]) <= 1e-12


def minimiser_distance(noise):
    scene, ref = cases.scene("rays", noise), cases.reference("rays", noise)
    off = scene["offsets"]
    truth = np.array([cases.minimiser_mp(scene["centers"][off[t]:off[t + 1]], scene["bearings"][off[t]:off[t + 1]], ref["points"][t])
                      for t in range(len(off) - 1)])
    return cases.relative_difference(ref["points"], truth)


def test_restatement_against_the_50_digit_minimiser():
    """the refined points of the noisy ray scenes against the minimiser of sum |normalize(X - o_i) - w_i|^2: TinySolver stops on an absolute
    cost change of 1e-6, after one step (noise 1e-3) or two (noise 0.03), so it is close to the minimiser, not at it"""
    each = [minimiser_distance(1e-3), minimiser_distance(0.03)]
    worst = max(each)
    print("noise 1e-3: %.3g, noise 0.03: %.3g" % tuple(each))
    print("largest relative distance between the restatement and the 50-digit minimiser: %.3g" % worst)
    assert worst <= cases.MINIMISER_RTOL
    assert cases.MINIMISER_RTOL == 10 * cases.MEASURED_MINIMISER_DISTANCE


def test_refinement_moves_towards_the_minimiser():
    """the midpoint (0 iterations) is further from the minimiser than the refined point"""
    scene, ref = cases.scene("rays", 0.03), cases.reference("rays", 0.03)
    off = scene["offsets"]
    worse = 0
    for t in range(16):
        o, w = scene["centers"][off[t]:off[t + 1]], scene["bearings"][off[t]:off[t + 1]]
        best = cases.minimiser_mp(o, w, ref["points"][t])
        worse += np.linalg.norm(cases.midpoint(o, w) - best) > np.linalg.norm(ref["points"][t] - best)
    assert worse >= 14


# ---- arguments ----
def test_emulated_edge_cases(emu):
    from opensfm_amd import _lib, reconstruction

    launches = emu.hipemu_launch_count
    launches.restype = C.c_long
    before = launches()
    points, status, iterations, _ = reconstruction.triangulate_bearings_arrays(np.zeros((0, 3)), np.zeros((0, 3)), [0])
    assert len(points) == 0 and len(status) == 0 and len(iterations) == 0
    scene = cases.scene("ragged", 65)
    points, _, _, _ = reconstruction.triangulate_tracks_arrays(scene["shot_pose"], scene["shot_camera"], scene["cam_model"], scene["cam_params"],
                                                               np.zeros(0, np.int32), np.zeros((0, 2)), [0])
    assert len(points) == 0 and launches() == before  # n_tracks == 0: no launch
    rays = cases.scene("special")
    o, w, off = rays["centers"], rays["bearings"], rays["offsets"]
    invalid = r"\(-1\)"  # OSFM_E_INVALID
    with pytest.raises(_lib.OsfmError, match=invalid):
        reconstruction.triangulate_bearings_arrays(o, w, off, refinement_iterations=-1)
    for angle in (-0.5, 180.5, float("nan")):
        with pytest.raises(_lib.OsfmError, match=invalid):
            reconstruction.triangulate_bearings_arrays(o, w, off, min_angle_deg=angle)
    bad = off.copy()
    bad[2], bad[3] = bad[3], bad[2]  # still ends at the number of rows, but decreases
    with pytest.raises(_lib.OsfmError, match=invalid):
        reconstruction.triangulate_bearings_arrays(o, w, bad)

    def tracks(**changes):
        s = dict(scene, **changes)
        return reconstruction.triangulate_tracks_arrays(s["shot_pose"], s["shot_camera"], s["cam_model"], s["cam_params"], s["obs_shot"], s["obs_xy"],
                                                        s["offsets"])

    for shot in (-1, len(scene["shot_pose"])):
        obs_shot = scene["obs_shot"].copy()
        obs_shot[40] = shot
        with pytest.raises(_lib.OsfmError, match=invalid):
            tracks(obs_shot=obs_shot)
    shot_camera = scene["shot_camera"].copy()
    shot_camera[3] = 2
    with pytest.raises(_lib.OsfmError, match=re.escape("(-1): osfm_triangulate_tracks: shot 3 names a camera outside the table") + "$"):
        tracks(shot_camera=shot_camera)
    with pytest.raises(_lib.OsfmError, match=re.escape("(-1): osfm_triangulate_tracks: camera 1 has model 10") + "$"):
        tracks(cam_model=np.array([0, 10], np.int32))

    def robust_tracks(**changes):
        s = dict(scene, **changes)
        return reconstruction.triangulate_tracks_arrays_robust(s["shot_pose"], s["shot_camera"], s["cam_model"], s["cam_params"], s["obs_shot"],
                                                               s["obs_xy"], s["offsets"], seed=1)

    with pytest.raises(_lib.OsfmError, match=re.escape("(-1): osfm_triangulate_tracks_robust: shot 3 names a camera outside the table") + "$"):
        robust_tracks(shot_camera=shot_camera)
    with pytest.raises(_lib.OsfmError, match=re.escape("(-1): osfm_triangulate_tracks_robust: camera 1 has model 10") + "$"):
        robust_tracks(cam_model=np.array([0, 10], np.int32))
    for value in (np.nan, np.inf):
        obs_xy = scene["obs_xy"].copy()
        obs_xy[-1, 1] = value  # in the 300-observation track: the wavefront kernel finds it
        with pytest.raises(_lib.OsfmError, match=invalid):
            tracks(obs_xy=obs_xy)
        shot_pose = scene["shot_pose"].copy()
        shot_pose[scene["obs_shot"][5], 10] = value  # used by a short track: the group kernel finds it
        with pytest.raises(_lib.OsfmError, match=invalid):
            tracks(shot_pose=shot_pose)


def test_emulated_not_finite_result_is_status_5(emu):
    """min_angle_deg = 0 and parallel rays: the midpoint's matrix is singular.  The reference would store the NaN point; this call says 5."""
    from opensfm_amd import reconstruction

    o = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    w = np.array([[0.0, 0, 1.0]] * 3)
    points, status, _, _ = reconstruction.triangulate_bearings_arrays(o, w, [0, 3], min_angle_deg=0.0)
    assert status[0] == 5 and np.isnan(points[0]).all()
    assert cases.restate_track(o, w, dict(cases.DEFAULT, min_angle_deg=0.0))[0] == 5


def test_emulated_track_longer_than_the_lds_slice(emu):
    """600 rays: the wavefront kernel keeps 512 in LDS and loads the rest again"""
    from opensfm_amd import reconstruction

    rng = np.random.default_rng(5)
    X = np.array([0.5, -0.3, 9.0])
    o = np.c_[rng.uniform(-4, 4, 600), rng.uniform(-4, 4, 600), rng.uniform(-1, 1, 600)]
    w = X - o + rng.normal(0, 1e-3, o.shape)
    w /= np.linalg.norm(w, axis=1)[:, None]
    scene = {"params": cases.DEFAULT, "offsets": np.array([0, 600, 602], np.int64), "centers": np.r_[o, o[:2]], "bearings": np.r_[w, w[:2]]}
    cases.check(cases.run_bearings(scene), cases.restatement(scene))
    assert reconstruction.TRIANGULATION_STATUS[0] == "triangulated"


# ---- the Python drop-ins ----
CONFIG = {"triangulation_threshold": 0.006, "triangulation_min_ray_angle": 1.0, "triangulation_min_depth": 0.001,
          "triangulation_refinement_iterations": 10, "triangulation_type": "FULL"}


def check_map(r, expected):
    assert set(r.points) == set(expected)
    for lm_id, (X, shots) in expected.items():
        assert np.linalg.norm(r.points[lm_id].coordinates - X) <= cases.POINT_RTOL * np.linalg.norm(X)
        assert {s for s, shot in r.shots.items() if lm_id in shot.observations} == shots
        assert r.points[lm_id].number_of_observations() == len(shots)


def check_python_dropins():
    """triangulate_shot_features and retriangulate over a reconstruction with rigs, through whatever library _lib.load() gives, against a
    per-track Python loop over the restatement: the same point ids, coordinates and observation sets"""
    from opensfm_amd import reconstruction

    r, manager = cases.rig_reconstruction()
    seen = ["s003", "s004", "ghost", "nowhere"]
    wanted = list(dict.fromkeys(t for s in seen if s in manager.get_shot_ids() for t in manager.get_shot_observations(s)))
    expected = cases.expected_map(r, manager, wanted)
    assert 10 < len(expected) < len(wanted)
    assert reconstruction.triangulate_shot_features(manager, r, set(seen), CONFIG) is None
    check_map(r, expected)
    # a second call over more shots adds only what is new and leaves the points that exist alone
    kept = {lm_id: r.points[lm_id] for lm_id in r.points}
    more = seen + ["s000", "s010"]
    wanted2 = list(dict.fromkeys(t for s in more if s in manager.get_shot_ids() for t in manager.get_shot_observations(s)))
    expected2 = dict(cases.expected_map(r, manager, [t for t in wanted2 if t not in kept]), **expected)
    reconstruction.triangulate_shot_features(manager, r, set(more), CONFIG)
    check_map(r, expected2)
    assert all(r.points[lm_id] is lm for lm_id, lm in kept.items()) and "lonely" not in r.points
    # retriangulate: everything the reconstruction's shots see
    before = len(r.points)
    everything = list(dict.fromkeys(t for s in r.shots if s in manager.get_shot_ids() for t in manager.get_shot_observations(s)))
    expected3 = cases.expected_map(r, manager, everything)
    report = reconstruction.retriangulate(manager, r, CONFIG)
    check_map(r, expected3)
    assert report["num_points_before"] == before and report["num_points_after"] == len(expected3) > before and report["wall_time"] > 0
    for shot in r.shots.values():
        assert set(shot.observations) <= set(expected3)


def test_emulated_python_dropins(emu):
    check_python_dropins()


def test_robust_raises_and_keys_are_required(emu):
    from opensfm_amd import reconstruction

    r, manager = cases.rig_reconstruction()
    reconstruction.triangulate_shot_features(manager, r, {"s003"}, CONFIG)
    n = len(r.points)
    assert n > 0
    with pytest.raises(NotImplementedError):
        reconstruction.triangulate_shot_features(manager, r, {"s004"}, dict(CONFIG, triangulation_type="ROBUST"))
    with pytest.raises(NotImplementedError):
        reconstruction.retriangulate(manager, r, dict(CONFIG, triangulation_type="ROBUST"))
    for key in CONFIG:
        config = {k: v for k, v in CONFIG.items() if k != key}
        with pytest.raises(KeyError):
            reconstruction.triangulate_shot_features(manager, r, {"s004"}, config)
        with pytest.raises(KeyError):
            reconstruction.retriangulate(manager, r, config)
    assert len(r.points) == n  # nothing above touched the map


def check_pygeometry_leaves():
    """compat.pygeometry under the reference's own test literals, and point_refinement against the restatement"""
    from opensfm_amd import compat
    from opensfm_amd.compat import pygeometry

    assert "pygeometry" not in compat.MODULES
    sc = cases.scene("ref_midpoint")
    ok, X = pygeometry.triangulate_bearings_midpoint(sc["centers"][:2], sc["bearings"][:2], 2 * [0.01], np.radians(2.0), 0.001)
    assert ok is True and np.allclose(X, [0, 0, 1.0])
    ok, X = pygeometry.triangulate_bearings_midpoint(sc["centers"][2:], sc["bearings"][2:], 2 * [0.01], np.radians(2.0), 0.001)
    assert ok is False
    ok, _ = pygeometry.triangulate_bearings_midpoint(sc["centers"][:2], sc["bearings"][:2], [0.01], np.radians(2.0), 0.001)
    assert ok is False  # a threshold list shorter than the rows
    with pytest.raises(NotImplementedError):
        pygeometry.triangulate_bearings_midpoint(sc["centers"][:2], sc["bearings"][:2], [0.01, 0.02], np.radians(2.0), 0.001)
    noisy = cases.scene("rays", 0.03)
    off = noisy["offsets"]
    for t in (0, 3, 6, 20):
        o, w = noisy["centers"][off[t]:off[t + 1]], noisy["bearings"][off[t]:off[t + 1]]
        ok, X = pygeometry.triangulate_bearings_midpoint(o, w, len(o) * [0.3], np.radians(1.0), 0.001)
        mid = cases.midpoint(o, w)
        assert ok is True and np.linalg.norm(X - mid) <= cases.POINT_RTOL * np.linalg.norm(mid)
        for iterations in (0, 1, 2, 10):
            want, _ = cases.refine(o, w, mid, iterations)
            got = pygeometry.point_refinement(o, w, mid, iterations)
            assert np.linalg.norm(got - want) <= cases.POINT_RTOL * np.linalg.norm(want)
        assert np.array_equal(pygeometry.point_refinement(o, w, mid, 0), mid) and np.array_equal(pygeometry.point_refinement(o, w, mid, 1), mid)


def test_emulated_pygeometry_leaves(emu):
    check_pygeometry_leaves()


def test_tracks_manager():
    from opensfm_amd.geometry_types import Observation, TracksManager

    m = TracksManager()
    a, b = Observation(0.1, 0.2, 1.0), Observation(0.3, 0.4, 1.0)
    m.add_observation("im1", "t1", a)
    m.add_observation("im2", "t1", b)
    m.add_observation("im2", "t2", a)
    assert m.get_shot_ids() == ["im1", "im2"] and m.get_track_ids() == ["t1", "t2"]
    assert m.get_observation("im2", "t1") is b and list(m.get_track_observations("t1")) == ["im1", "im2"]
    assert list(m.get_shot_observations("im2")) == ["t1", "t2"] and m.get_track_observations("t1")["im1"].point[1] == 0.2


# ---- a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer ----
def test_sanitised_program_on_the_ragged_scene(emu, tmp_path):
    """tests/native/triangulate_main.cpp (its own main, linked with the emulated triangulate.hip under -fsanitize=address,undefined) on the
    ragged scene with every boundary length: a clean exit, and the same bits as the unsanitised emulation"""
    exe = _builder().build_main()
    scene = cases.scene("ragged", 65)
    o, w = cases.rays_of(scene)
    p = scene["params"]
    n_tracks, n_obs = len(scene["offsets"]) - 1, len(scene["obs_shot"])
    path, out = str(tmp_path / "scene.bin"), str(tmp_path / "result.bin")
    with open(path, "wb") as f:
        f.write(np.array([n_tracks, len(scene["shot_pose"]), len(scene["cam_model"]), 0], np.int32).tobytes())
        f.write(np.array([n_obs], np.int64).tobytes())
        f.write(np.array([p["threshold"], p["min_angle_deg"], p["min_depth"]], np.float64).tobytes())
        f.write(np.array([p["iterations"], 0], np.int32).tobytes())
        for a, t in ((scene["offsets"], np.int64), (scene["shot_pose"], np.float64), (scene["shot_camera"], np.int32), (scene["cam_model"], np.int32),
                     (scene["cam_params"], np.float64), (scene["obs_shot"], np.int32), (scene["obs_xy"], np.float64), (o, np.float64), (w, np.float64)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, path, out], env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-4000:]
    assert "Sanitizer" not in done.stderr and "runtime error" not in done.stderr, done.stderr[-4000:]
    raw = open(out, "rb").read()
    per = n_tracks * (24 + 1 + 4)
    assert len(raw) == 2 * per
    for entry, run in enumerate((cases.run_tracks, cases.run_bearings)):
        blob = raw[entry * per:(entry + 1) * per]
        points = np.frombuffer(blob[:n_tracks * 24], np.float64).reshape(-1, 3)
        status = np.frombuffer(blob[n_tracks * 24:n_tracks * 25], np.uint8)
        iterations = np.frombuffer(blob[n_tracks * 25:], np.int32)
        want = run(scene)
        assert np.array_equal(points, want[0], equal_nan=True) and np.array_equal(status, want[1]) and np.array_equal(iterations, want[2])
