"""The robust track triangulation of ``opensfm_amd/csrc/triangulate.hip`` (``triangulation_type: ROBUST``) without a GPU: the kernels on the
host emulation of HIP (``tests/native/build_triangulate_emu.py``) against the step-by-step restatement of
``tests/triangulate_robust_cases.py``, the restatement against the reference's own ``TrackTriangulator.triangulate_robust`` (where the
reference is mounted), the unranking and the generator of ``triangulate_robust.h`` against ``itertools.combinations`` and Python integers,
the keyworded Python drop-ins against a per-track loop, and a stand-alone sanitised program over the rays scene."""
import contextlib
import ctypes as C
import importlib.util
import itertools
import os
import subprocess

import numpy as np
import pytest

import triangulate_cases as full_cases
import triangulate_robust_cases as cases

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


@pytest.fixture(scope="module")
def program():
    """the stand-alone program (sanitised; its own main)"""
    return _builder().build_main("triangulate_robust_main")


def run_program(exe, args, text=None):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe] + args, env=env, input=text, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-4000:]
    assert "Sanitizer" not in done.stderr and "runtime error" not in done.stderr, done.stderr[-4000:]
    return done.stdout


# ---- the restatement alone ----
@pytest.mark.parametrize("kind,how", cases.ALL_RUNS)
def test_no_scene_has_a_borderline_comparison(kind, how):
    """the condition under which the discrete outputs must be identical: no chord-vs-threshold, optimal_iter-vs-index or solver comparison
    of the restatement within 1e-9 relative of its bound (a seed that gives one is replaced, the comparison is never loosened)"""
    assert cases.reference(kind, how)["borderline"] == []


def test_scenes_cover_the_lengths_and_every_outcome():
    lengths = np.diff(cases.scene("rays")["offsets"]).tolist()
    assert len(lengths) == cases.N_RAYS and set(cases.LENGTHS) <= set(lengths)
    for how in ("explicit", "seeded"):
        ref = cases.reference("rays", how)
        assert {0, 1, 6} <= set(ref["status"].tolist())
        words = {w for log in ref["log"] for w in log}
        assert {"repeat", "invalid", "not better"} <= words and any(w.startswith("ls wins") for w in words) and any(w.startswith("ls loses") for w in words)
        assert (ref["n_inliers"][ref["status"] == 0] >= 2).all() and ref["tries"].max() == cases.TRIES
        long = [t for t, n in enumerate(lengths) if n > 512]
        off = cases.scene("rays")["offsets"]
        past = np.concatenate([ref["mask"][off[t] + 512:off[t + 1]] for t in long])  # the rows a wavefront does not keep in LDS
        assert len(long) == 4 and all(ref["status"][t] == 0 for t in long) and 0 < past.sum() < len(past)
    assert "obs_xy" in cases.scene("pixels") and (cases.reference("pixels", "explicit")["status"] == 0).sum() > 50


def test_hand_made_draws_take_each_branch():
    """tries_used and the branch log of the restatement say that every hand-made track does what it was made for"""
    sc, ref = cases.scene("forced"), cases.reference("forced", "explicit")
    log = dict(zip(sc["names"], ref["log"]))
    row = {name: k for k, name in enumerate(sc["names"])}
    assert log["repeated id"][:2] == ["ls loses, goes on", "repeat"]
    assert log["all inliers on the first try"] == ["ls loses, all inliers"] and ref["n_inliers"][row["all inliers on the first try"]] == 10
    # 7 of 10: log(0.01) / log(1 - 0.49) = 6.84 <= 7 stops after one try, <= 3 does not
    assert log["enough by the first index"] == ["ls loses, enough"] and ref["tries"][row["enough by the first index"]] == 1
    assert ref["n_inliers"][row["enough by the first index"]] == 7
    assert log["small first index goes on"][0] == "ls loses, goes on" and ref["tries"][row["small first index goes on"]] > 1
    assert log["subset refinement wins"][0].startswith("ls wins")
    assert log["subset refinement loses"][0].startswith("ls loses")
    assert set(log["every try invalid"]) <= {"invalid", "repeat"} and len(log["every try invalid"]) == cases.TRIES
    assert ref["status"][row["every try invalid"]] == 6 and ref["tries"][row["every try invalid"]] == cases.TRIES
    # u = 1 - 2^-53 and C = 45: id = 43 = C - 2, the pair (7, 9); the last pair (8, 9) holds a wrong ray and would not give 7 inliers at once
    assert int((1.0 - 2.0 ** -53) * 44) == 43 and cases.unrank(43, 10) == (7, 9)
    k = row["u next to 1"]
    assert log["u next to 1"] == ["ls loses, enough"] and ref["n_inliers"][k] == 7
    assert list(ref["mask"][sc["offsets"][k]:sc["offsets"][k + 1]]) == [0, 0, 1, 1, 1, 1, 1, 1, 0, 1]
    assert (ref["status"] == [0, 0, 0, 0, 0, 0, 6, 0]).all()


def test_unrank_restatement_is_itertools_order():
    for n in range(2, 13):
        assert [cases.unrank(r, n) for r in range(n * (n - 1) // 2)] == list(itertools.combinations(range(n), 2))


# ---- the host side of triangulate_robust.h: unranking and generator ----
def test_unranking_is_exact(program):
    """every id of n <= 12 against itertools.combinations; the first, the last and the ids around every row boundary probed of n = 2^24
    against integer arithmetic"""
    asked, want = [], []
    for n in range(2, 13):
        for rank, pair in enumerate(itertools.combinations(range(n), 2)):
            asked.append((n, rank))
            want.append(pair)
    n = 1 << 24
    before = lambda i: i * (2 * n - i - 1) // 2  # noqa: E731  (pairs with a first index below i)
    rows = [0, 1, 2, 3, 1000, 4096, 65535, 65536, 1 << 20, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, 12345678, n - 4097, n - 1025, n - 5, n - 4, n - 3, n - 2]
    for i in rows:
        first, last = before(i), before(i + 1) - 1
        for rank in {first, min(first + 1, last), last - 1 if last > first else last, last}:
            asked.append((n, rank))
            want.append((i, i + 1 + rank - first))
    assert (n, 0) in asked and (n, n * (n - 1) // 2 - 1) in asked
    out = run_program(program, ["--unrank"], "".join("%d %d\n" % a for a in asked))
    got = [tuple(int(v) for v in line.split()) for line in out.split("\n") if line]
    assert got == want


def test_generator_equals_its_integer_restatement(program):
    asked = [(seed, t, k) for seed in (0, 1, cases.SEED, 2 ** 63, 2 ** 64 - 1) for t in (0, 1, 7, 299, 499999, 2 ** 31 - 1) for k in (0, 1, 10)]
    out = run_program(program, ["--draw"], "".join("%d %d %d\n" % a for a in asked))
    got = [float.fromhex(line) for line in out.split("\n") if line]
    want = [cases.draw(*a) for a in asked]
    assert got == want and all(0.0 <= u < 1.0 for u in want)
    many = cases.seeded_draws(cases.SEED, 2000).reshape(-1)
    assert 0.49 < many.mean() < 0.51 and len(set(many.tolist())) == len(many)


# ---- the kernels on the CPU against the restatement ----
_RESULTS = {}


def emulated_result(kind, how, entry):
    """one emulated run per scene, draws and entry point, shared by the tests below (call with the `emu` fixture active)"""
    key = (kind, how, entry)
    if key not in _RESULTS:
        _RESULTS[key] = cases.run(entry, kind, how)
    return _RESULTS[key]


def entries(kind):
    return ("bearings", "tracks") if "obs_xy" in cases.scene(kind) else ("bearings",)


@pytest.mark.parametrize("kind,how", cases.ALL_RUNS)
def test_emulated_scene_equals_the_restatement(emu, kind, how):
    """identical status, inlier mask, inlier count and tries, points within POINT_RTOL, through both entry points"""
    ref = cases.reference(kind, how)
    for entry in entries(kind):
        cases.check(emulated_result(kind, how, entry), ref)


def test_point_tolerance_is_100_times_the_measured_difference(emu):
    worst = 0.0
    for kind, how in cases.ALL_RUNS:
        for entry in entries(kind):
            worst = max(worst, full_cases.relative_difference(emulated_result(kind, how, entry)[0], cases.reference(kind, how)["points"]))
    print("largest relative difference between the emulated robust kernels and the restatement: %.3g" % worst)
    assert worst <= cases.MEASURED_POINT_DIFFERENCE  # a larger value means the constant has to be measured again
    assert cases.POINT_RTOL == 100 * cases.MEASURED_POINT_DIFFERENCE


def test_emulated_seeded_run_equals_the_same_draws_given(emu):
    """the device's generator gives the bits of its restatement: a seeded run and a run fed seeded_draws() are byte-equal"""
    sc = cases.scene("rays")
    seeded = emulated_result("rays", "seeded", "bearings")
    given = cases.run_bearings(sc, draws=cases.draws_of("rays", "seeded"))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(seeded[:5], given[:5]))


def test_emulated_tracks_do_not_depend_on_their_neighbours(emu):
    """a track alone in a call with its own draws gives the bits it gives inside the batch"""
    sc, draws = cases.scene("rays"), cases.draws_of("rays", "explicit")
    batch = emulated_result("rays", "explicit", "bearings")
    off = sc["offsets"]
    for t in (2, 9, 13, 14, 40):
        one = dict(sc, offsets=np.array([0, off[t + 1] - off[t]], np.int64), centers=sc["centers"][off[t]:off[t + 1]], bearings=sc["bearings"][off[t]:off[t + 1]])
        alone = cases.run_bearings(one, draws=draws[t:t + 1])
        assert alone[0].tobytes() == batch[0][t:t + 1].tobytes() and alone[1][0] == batch[1][t] and alone[4][0] == batch[4][t]
        assert alone[2].tobytes() == batch[2][off[t]:off[t + 1]].tobytes()


def check_edge_cases(ctx=None):
    """empty input, only-empty tracks, bad draws and bad offsets: refused with OSFM_E_INVALID, and the context still works afterwards"""
    from opensfm_amd import _lib, reconstruction

    out = reconstruction.triangulate_bearings_arrays_robust(np.zeros((0, 3)), np.zeros((0, 3)), [0], ctx=ctx)
    assert all(len(a) == 0 for a in out[:5]) and out[5] == 0.0
    px = cases.scene("pixels")
    out = reconstruction.triangulate_tracks_arrays_robust(px["shot_pose"], px["shot_camera"], px["cam_model"], px["cam_params"], np.zeros(0, np.int32),
                                                          np.zeros((0, 2)), [0], ctx=ctx)
    assert all(len(a) == 0 for a in out[:5])
    points, status, mask, n_inliers, tries, _ = reconstruction.triangulate_bearings_arrays_robust(np.zeros((0, 3)), np.zeros((0, 3)), [0, 0, 0], seed=5, ctx=ctx)
    assert list(status) == [1, 1] and np.isnan(points).all() and len(mask) == 0 and list(n_inliers) == [0, 0] and list(tries) == [0, 0]
    sc = cases.scene("forced")
    o, w, off, draws = sc["centers"], sc["bearings"], sc["offsets"], sc["draws"]
    invalid = r"\(-1\)"  # OSFM_E_INVALID
    for value in (1.0, -1e-9, 1.5, np.nan, np.inf):
        for row, col in ((0, 10), (len(draws) - 1, 0)):  # (a draw the walk would never reach counts too)
            bad = draws.copy()
            bad[row, col] = value
            with pytest.raises(_lib.OsfmError, match=invalid):
                reconstruction.triangulate_bearings_arrays_robust(o, w, off, draws=bad, ctx=ctx)
    long = cases.scene("rays")
    first_long = int(np.flatnonzero(np.diff(long["offsets"]) > 32)[0])
    bad = cases.draws_of("rays", "explicit").copy()
    bad[first_long, 3] = 1.0  # found by the wavefront kernel
    with pytest.raises(_lib.OsfmError, match=invalid):
        cases.run_bearings(long, draws=bad, ctx=ctx)
    with pytest.raises(ValueError):
        reconstruction.triangulate_bearings_arrays_robust(o, w, off, draws=draws[:-1], ctx=ctx)
    swapped = off.copy()
    swapped[2], swapped[3] = swapped[3], swapped[2]  # still ends at the number of rows, but decreases
    with pytest.raises(_lib.OsfmError, match=invalid):
        reconstruction.triangulate_bearings_arrays_robust(o, w, swapped, draws=draws, ctx=ctx)
    shifted = off.copy()
    shifted[0] = 1
    with pytest.raises(_lib.OsfmError, match=invalid):
        reconstruction.triangulate_bearings_arrays_robust(o, w, shifted, draws=draws, ctx=ctx)
    with pytest.raises(_lib.OsfmError, match=invalid):
        reconstruction.triangulate_bearings_arrays_robust(o, w, off, draws=draws, refinement_iterations=-1, ctx=ctx)
    obs_shot = px["obs_shot"].copy()
    obs_shot[7] = len(px["shot_pose"])  # the kernel must refuse it without reading the pose table there
    with pytest.raises(_lib.OsfmError, match=invalid):
        cases.run_tracks(dict(px, obs_shot=obs_shot), seed=1, ctx=ctx)
    cases.check(cases.run_bearings(sc, draws=draws, ctx=ctx), cases.reference("forced", "explicit"))  # the context still works


def test_emulated_edge_cases(emu):
    check_edge_cases()


# ---- the Python drop-ins ----
CONFIG = {"triangulation_threshold": 0.006, "triangulation_min_ray_angle": 1.0, "triangulation_min_depth": 0.001,
          "triangulation_refinement_iterations": 10, "triangulation_type": "ROBUST"}
ROBUST_SEED, RETRIANGULATE_SEED = 9, 11  # (seeds under which expected_map meets no borderline comparison)


def check_map(r, expected):
    assert set(r.points) == set(expected)
    for lm_id, (X, shots) in expected.items():
        assert np.linalg.norm(r.points[lm_id].coordinates - X) <= cases.POINT_RTOL * np.linalg.norm(X)
        assert {s for s, shot in r.shots.items() if lm_id in shot.observations} == shots
        assert r.points[lm_id].number_of_observations() == len(shots)


def check_python_dropins():
    """triangulate_shot_features and retriangulate with robust_seed / robust_draws over a reconstruction with rigs, through whatever
    library _lib.load() gives, against a per-track Python loop over the restatement: the same point ids, coordinates and INLIER sets;
    track k of the call's track list draws as track k"""
    from opensfm_amd import reconstruction

    r, manager = full_cases.rig_reconstruction()
    seen = ["s003", "s004", "ghost", "nowhere"]
    wanted = list(dict.fromkeys(t for s in seen if s in manager.get_shot_ids() for t in manager.get_shot_observations(s)))
    expected = cases.expected_map(r, manager, wanted, ROBUST_SEED)
    assert 10 < len(expected) <= len(wanted)
    assert reconstruction.triangulate_shot_features(manager, r, seen, CONFIG, robust_seed=ROBUST_SEED) is None
    check_map(r, expected)
    # some point is observed by fewer shots than its track has in the reconstruction: only the inliers were added
    in_map = {t: sum(s in r.shots for s in manager.get_track_observations(t)) for t in expected}
    assert any(len(shots) < in_map[t] for t, (_, shots) in expected.items())
    # robust_draws: row k for track k; the generator's own values give the same map
    r2, _ = full_cases.rig_reconstruction()
    reconstruction.triangulate_shot_features(manager, r2, seen, CONFIG, robust_draws=cases.seeded_draws(ROBUST_SEED, len(wanted)))
    check_map(r2, expected)
    with pytest.raises(ValueError):
        reconstruction.triangulate_shot_features(manager, r2, ["s010"], CONFIG, robust_draws=np.zeros((1, 11)))
    with pytest.raises(ValueError):
        reconstruction.triangulate_shot_features(manager, r2, ["s010"], CONFIG, robust_seed=1, robust_draws=np.zeros((1, 11)))
    # retriangulate: everything the reconstruction's shots see
    before = len(r.points)
    everything = list(dict.fromkeys(t for s in r.shots if s in manager.get_shot_ids() for t in manager.get_shot_observations(s)))
    expected3 = cases.expected_map(r, manager, everything, RETRIANGULATE_SEED)
    report = reconstruction.retriangulate(manager, r, CONFIG, robust_seed=RETRIANGULATE_SEED)
    check_map(r, expected3)
    assert report["num_points_before"] == before and report["num_points_after"] == len(expected3) > before
    for shot in r.shots.values():
        assert set(shot.observations) <= set(expected3)


def test_emulated_python_dropins(emu):
    check_python_dropins()


def test_robust_without_the_keywords_still_raises(emu):
    """neither keyword: NotImplementedError before the map is touched, with a message that names the two keywords; FULL ignores them"""
    from opensfm_amd import reconstruction

    r, manager = full_cases.rig_reconstruction()
    full = dict(CONFIG, triangulation_type="FULL")
    reconstruction.triangulate_shot_features(manager, r, {"s003"}, full)
    n = len(r.points)
    assert n > 0
    with pytest.raises(NotImplementedError, match="robust_seed.*robust_draws"):
        reconstruction.triangulate_shot_features(manager, r, {"s004"}, CONFIG)
    with pytest.raises(NotImplementedError, match="robust_seed.*robust_draws"):
        reconstruction.retriangulate(manager, r, CONFIG)
    assert len(r.points) == n
    a, _ = full_cases.rig_reconstruction()
    b, _ = full_cases.rig_reconstruction()
    reconstruction.triangulate_shot_features(manager, a, ["s003", "s004"], full)
    reconstruction.triangulate_shot_features(manager, b, ["s003", "s004"], full, robust_seed=3)
    assert list(a.points) == list(b.points) and all(np.array_equal(a.points[k].coordinates, b.points[k].coordinates) for k in a.points)
    assert all(set(a.shots[s].observations) == set(b.shots[s].observations) for s in a.shots)


# ---- the restatement against the reference's own code ----
class _RayShot:
    """a shot that is one ray: origin o, identity rotation, and a camera whose bearing of the observation's `point` is the point itself"""

    def __init__(self, shot_id, origin):
        self.id, self.origin = shot_id, origin
        self.pose = self.camera = self

    def get_origin(self):
        return self.origin

    def get_rotation_matrix(self):
        return np.eye(3)

    def pixel_bearing(self, point):
        return np.array(point, np.float64)


class _RayObservation:
    def __init__(self, point):
        self.point = point


@pytest.mark.parametrize("kind,how", [("rays", "explicit"), ("forced", "explicit"), ("rays", "seeded")])
def test_restatement_equals_the_reference_code(emu, monkeypatch, kind, how):
    """TrackTriangulator.triangulate_robust of the reference itself, track by track: its pygeometry is opensfm_amd.compat.pygeometry on the
    emulation, np.random.rand pops the track's draws, a small TrackHandlerBase records what it stores.  The same point ids and inlier
    sets as the restatement, points within POINT_RTOL: the shadowed `i`, the `C - 1`, the `continue` and the dead midpoint are pinned
    against the real thing."""
    import bundle_cases
    from opensfm_amd.compat import pygeometry

    ref_mod = bundle_cases.load_reference_reconstruction()
    if ref_mod is None:
        pytest.skip("the reference is not mounted")
    ref_mod.pygeometry = pygeometry
    sc, draws, want = cases.scene(kind), cases.draws_of(kind, how), cases.reference(kind, how)
    off, p = sc["offsets"], sc["params"]

    class Shots(dict):
        pass

    class Holder:
        shots = Shots()

    class Handler(ref_mod.TrackHandlerBase):
        def __init__(self):
            self.points, self.inliers = {}, {}

        def get_observations(self, track_id):
            t = int(track_id)
            return {str(k): _RayObservation(sc["bearings"][k]) for k in range(off[t], off[t + 1])}

        def store_track_coordinates(self, track_id, coordinates):
            self.points[int(track_id)] = np.array(coordinates, np.float64)

        def store_inliers_observation(self, track_id, shot_id):
            self.inliers.setdefault(int(track_id), []).append(int(shot_id))

    for k in range(len(sc["centers"])):
        Holder.shots[str(k)] = _RayShot(str(k), sc["centers"][k])
    handler = Handler()
    triangulator = ref_mod.TrackTriangulator(Holder, handler)
    consumed = []
    for t in range(len(off) - 1):
        pending = list(draws[t])
        monkeypatch.setattr(np.random, "rand", lambda: pending.pop(0))
        triangulator.triangulate_robust(str(t), p["threshold"], p["min_angle_deg"], p["min_depth"], p["iterations"])
        consumed.append(cases.TRIES - len(pending))
    monkeypatch.undo()
    assert sorted(handler.points) == np.flatnonzero(want["status"] == 0).tolist()
    assert consumed == want["tries"].tolist()
    for t, X in handler.points.items():
        assert sorted(handler.inliers[t]) == (off[t] + np.flatnonzero(want["mask"][off[t]:off[t + 1]])).tolist()
        assert np.linalg.norm(X - want["points"][t]) <= cases.POINT_RTOL * np.linalg.norm(want["points"][t])


# ---- a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer ----
def test_sanitised_program_on_the_rays_scene(emu, program, tmp_path):
    """tests/native/triangulate_robust_main.cpp (its own main, linked with the emulated triangulate.hip under -fsanitize=address,undefined) on
    the rays scene with every boundary length, with explicit and with seeded draws: a clean exit, and the bits of the unsanitised
    emulation.  Nothing sanitised is loaded into Python."""
    sc = cases.scene("rays")
    p, draws = sc["params"], cases.draws_of("rays", "explicit")
    n_tracks, n_obs = len(sc["offsets"]) - 1, len(sc["centers"])
    path, out = str(tmp_path / "scene.bin"), str(tmp_path / "result.bin")
    with open(path, "wb") as f:
        f.write(np.array([n_tracks, 0], np.int32).tobytes())
        f.write(np.array([n_obs], np.int64).tobytes())
        f.write(np.array([p["threshold"], p["min_angle_deg"], p["min_depth"]], np.float64).tobytes())
        f.write(np.array([p["iterations"], 0], np.int32).tobytes())
        f.write(np.array([cases.SEED], np.uint64).tobytes())
        for a, t in ((sc["offsets"], np.int64), (sc["centers"], np.float64), (sc["bearings"], np.float64), (draws, np.float64)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    run_program(program, [path, out])
    raw = open(out, "rb").read()
    per = n_tracks * (24 + 1 + 4 + 4) + n_obs
    assert len(raw) == 2 * per
    for run, how in enumerate(("explicit", "seeded")):
        blob = raw[run * per:(run + 1) * per]
        cuts = np.cumsum([0, n_tracks * 24, n_tracks, n_obs, n_tracks * 4, n_tracks * 4])
        parts = [np.frombuffer(blob[a:b], t) for a, b, t in zip(cuts[:-1], cuts[1:], (np.float64, np.uint8, np.uint8, np.int32, np.int32))]
        want = emulated_result("rays", how, "bearings")
        assert np.array_equal(parts[0].reshape(-1, 3), want[0], equal_nan=True)
        assert all(np.array_equal(a, b) for a, b in zip(parts[1:], want[1:5]))
