"""Absolute-pose LO-RANSAC of resect on the MI355X (abspose.hip): every result field and both masks equal to the host build of the same
header (tests/native/abspose_host.cpp) bit for bit; the pixels twin; compat.pyrobust.ransac_absolute_pose and the pygeometry leaves
against the reference tests' tolerances; reconstruction.resect / resect_candidates against a per-image loop over the host build on a
synthetic map; the documented errors."""
import copy
import re

import numpy as np
import pytest

import abspose_cases as cases
from test_abspose_host import THRESHOLD, build_host, host_images, host_images_threads, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return build_host()


@pytest.fixture(scope="module")
def batch():
    """~300 images: the sizes at which the walk changes path once, one image of 20 000 rows (longer than the LDS inlier list: the scratch
    path), the rest with 5 - 1 500 rows.  One image in 30 is all outliers: there nearly every model ties the best of 3 inliers and fires
    a local optimisation, the longest walk there is, so a few of them are enough."""
    rng = np.random.default_rng(0)

    def kind(k):
        name = cases.KINDS[k % len(cases.KINDS)]
        return name if name != "all_outliers" or k % 30 == 4 else "noisy"

    probs = [cases.make_problem(rng, n, kind(k), outliers=rng.uniform(0, 0.9)) for k, n in enumerate(cases.SIZES)]
    probs.append(cases.make_problem(rng, 20000, "noisy", outliers=0.2, noise=2e-4))
    while len(probs) < 300:
        n = int(np.exp(rng.uniform(np.log(5), np.log(1500))))
        probs.append(cases.make_problem(rng, n, kind(len(probs)), outliers=rng.uniform(0, 0.9), noise=rng.choice([2e-4, 1e-3])))
    rng.shuffle(probs)  # (the host build takes the images in equal runs, one per thread)
    return cases.pack(probs)


def _assert_equal(got, want, p):
    g, w = got[p], want[p]
    assert same_bits(g["model"], np.array(w.model)), p
    assert same_bits(g["lo_model"], np.array(w.lo_model)), p
    assert (g["score"], g["iterations"], g["num_inliers"]) == (w.score, w.iterations, w.num_inliers), p


def test_batch_equals_host_build_bit_for_bit(host, batch, gpu_ctx):
    from opensfm_amd import reconstruction

    b, X, off = batch
    assert (np.diff(off) > 4096).any() and len(off) - 1 >= 300
    got, rmask, cmask, ms = reconstruction.abspose_images(b, X, off, THRESHOLD, ctx=gpu_ctx)
    want, wrmask, wcmask = host_images_threads(host, b, X, off, THRESHOLD)
    assert ms > 0
    for p in range(len(want)):
        _assert_equal(got, want, p)
    assert np.array_equal(rmask, wrmask) and np.array_equal(cmask, wcmask)
    assert sum(w.iterations < 1000 for w in want) > 50 and sum(w.iterations == 1000 for w in want) >= 10
    again, rmask2, cmask2, _ = reconstruction.abspose_images(b, X, off, THRESHOLD, ctx=gpu_ctx)  # no atomics on floats: two runs agree
    for g, a in zip(got, again):
        assert same_bits(g["model"], a["model"]) and same_bits(g["lo_model"], a["lo_model"])
        assert (g["score"], g["iterations"], g["num_inliers"]) == (a["score"], a["iterations"], a["num_inliers"])
    assert np.array_equal(rmask, rmask2) and np.array_equal(cmask, cmask2)


def test_parameters_without_lo_and_reduction_equal_host(host, batch, gpu_ctx):
    from opensfm_amd import reconstruction

    b, X, off = batch
    got, rmask, cmask, _ = reconstruction.abspose_images(b, X, off, THRESHOLD, iterations=120, use_lo=False, use_iteration_reduction=False,
                                                         ctx=gpu_ctx)
    want, wrmask, wcmask = host_images(host, b, X, off, THRESHOLD, iterations=120, use_lo=0, use_reduction=0)
    for p in range(len(want)):
        _assert_equal(got, want, p)
        assert got[p]["iterations"] == 120
    assert np.array_equal(rmask, wrmask) and np.array_equal(cmask, wcmask)


def test_lo_longer_than_a_batch_equals_host(host, gpu_ctx):
    """70 local-optimisation iterations, one more than a batch of 64 Lu-Hager solves holds: a second batch per firing, and batches cut
    short where a sample changes the inlier list.  Rows around the minimal sample and the wavefront; no all-outliers image (its walk is
    the long one and takes no other path)."""
    from opensfm_amd import reconstruction

    rng = np.random.default_rng(21)
    kinds = [k for k in cases.KINDS if k != "all_outliers"]
    sizes = [3, 4, 5, 63, 64, 65, 300] * 3
    b, X, off = cases.pack([cases.make_problem(rng, n, kinds[k % len(kinds)], outliers=rng.uniform(0, 0.6)) for k, n in enumerate(sizes)])
    got, rmask, cmask, _ = reconstruction.abspose_images(b, X, off, THRESHOLD, iterations=60, lo_iterations=70, ctx=gpu_ctx)
    want, wrmask, wcmask = host_images(host, b, X, off, THRESHOLD, iterations=60, lo_iterations=70)
    for p in range(len(want)):
        _assert_equal(got, want, p)
    assert np.array_equal(rmask, wrmask) and np.array_equal(cmask, wcmask)
    assert sum(w.score >= 3 for w in want) >= 15  # a local optimisation fired in most of them


def test_pixels_twin_equals_bearings_call(gpu_ctx):
    """abspose_images_pixels == abspose_images fed with pixel_bearing_many's bearings, over four camera models"""
    from opensfm_amd import matching, reconstruction
    from test_gpu_relrot import _Cam, _project

    cameras = [_Cam("perspective", focal=0.9, k1=-0.05, k2=0.01),
               _Cam("brown", focal=0.85, aspect_ratio=1.02, k1=-0.03, k2=0.005, k3=0.0, p1=1e-3, p2=-5e-4, principal_point=(0.01, -0.02)),
               _Cam("fisheye", focal=0.6, k1=-0.02, k2=0.003), _Cam("spherical")]
    rng = np.random.default_rng(12)
    xy, Xs, bs, image_cam = [], [], [], []
    for k, n in enumerate([3, 40, 65, 300, 700, 64, 5, 1200]):
        b, X, _, _ = cases.make_problem(rng, n, "noisy", outliers=rng.uniform(0, 0.6))
        b[:, 2] = np.abs(b[:, 2])  # in front of the camera
        cam = cameras[k % 4]
        p = _project(cam, b)
        xy.append(p)
        Xs.append(X)
        bs.append(matching.pixel_bearing_many(cam, p, gpu_ctx))
        image_cam.append(k % 4)
    off = np.r_[0, np.cumsum([len(p) for p in xy])].astype(np.int64)
    table = [matching.camera_parameters(c) for c in cameras]
    got, rmask, cmask, ms = reconstruction.abspose_images_pixels(np.concatenate(xy), np.concatenate(Xs), off, np.array(image_cam, np.int32),
                                                                 np.array([t[0] for t in table], np.int32), np.array([t[1] for t in table]),
                                                                 THRESHOLD, ctx=gpu_ctx)
    want, wrmask, wcmask, _ = reconstruction.abspose_images(np.concatenate(bs), np.concatenate(Xs), off, THRESHOLD, ctx=gpu_ctx)
    assert ms > 0
    for g, w in zip(got, want):
        assert same_bits(g["model"], w["model"]) and same_bits(g["lo_model"], w["lo_model"])
        assert (g["score"], g["iterations"], g["num_inliers"]) == (w["score"], w["iterations"], w["num_inliers"])
    assert np.array_equal(rmask, wrmask) and np.array_equal(cmask, wcmask)
    assert sum(g["score"] > 10 for g in got) >= 5


def outlier_shots(seed=7, count=6, n=300):
    """test_robust.py::test_outliers_absolute_pose_ransac's inputs restaged: exact shots, uniform noise of 1e-3 on the bearings, 30 % of
    them moved by 0.1 - 1 per component"""
    rng = np.random.default_rng(seed)
    out = []
    for Rt, bearings, points in cases.exact_shots(seed=seed, count=count, n=n):
        scale = 1e-3
        bearings = bearings + rng.random(bearings.shape) * scale
        ratio_outliers = 0.3
        bad = rng.permutation(len(bearings))[: int(ratio_outliers * len(bearings))]
        bearings[bad] += rng.uniform(0.1, 1.0, (len(bad), 3)) * rng.choice([-1, 1], (len(bad), 3))
        bearings /= np.linalg.norm(bearings, axis=1)[:, None]
        out.append((Rt, bearings, points, scale, ratio_outliers))
    return out


def test_pyrobust_absolute_pose_reference_tolerances(gpu_ctx):
    """test_robust.py::test_outliers_absolute_pose_ransac restaged with this repo's data: inliers within 5 %, Frobenius < 8e-2"""
    from opensfm_amd.compat import pyrobust

    for expected, bearings, points, scale, ratio_outliers in outlier_shots():
        params = pyrobust.RobustEstimatorParams()
        params.iterations = 1000
        result = pyrobust.ransac_absolute_pose(bearings, points, scale, params, pyrobust.RansacType.RANSAC)
        tolerance = 0.05
        inliers_count = (1 - ratio_outliers) * len(points)
        assert np.isclose(len(result.inliers_indices), inliers_count, rtol=tolerance)
        assert np.linalg.norm(expected - result.lo_model, ord="fro") < 8e-2


def test_pygeometry_leaves_on_exact_data(gpu_ctx):
    """test_multiview.py::test_absolute_pose_three_points / ::test_absolute_pose_n_points restaged, with their bounds"""
    from opensfm_amd.compat import pygeometry

    shots = cases.exact_shots()
    exact_found = 0
    for expected, bearings, points in shots:
        result = pygeometry.absolute_pose_three_points(bearings, points)
        for Rt in result:
            exact_found += bool(np.linalg.norm(expected - Rt, ord="fro") < 1e-6)
    assert exact_found >= len(shots) - 2
    for expected, bearings, points in shots[:10]:
        result = pygeometry.absolute_pose_n_points(bearings, points)
        assert np.linalg.norm(expected - result, ord="fro") < 1e-5
    dup = shots[0][1].copy(), shots[0][2].copy()
    dup[0][1], dup[1][1] = dup[0][0], dup[1][0]
    assert pygeometry.absolute_pose_three_points(*dup) == []  # sigma == 0: no model


# ---- the drop-ins ----
def _host_resect(host, data, tracks_manager, reconstruction, shot_id, threshold, min_inliers, gpu_ctx):
    """resect (opensfm/reconstruction.py:695-762) line by line, the estimator served by the host build and the bearings by
    pixel_bearing_many"""
    from opensfm_amd import matching
    from opensfm_amd import reconstruction as rec_mod
    from opensfm_amd.geometry_types import Pose, RigInstance

    rig_assignments = {}
    for instance_id, instance in data.load_rig_assignments().items():
        for image, rig_camera_id in instance:
            rig_assignments[image] = (instance_id, rig_camera_id, [s[0] for s in instance])
    camera = reconstruction.cameras[data.load_exif(shot_id)["camera"]]
    xy, Xs, ids = [], [], []
    for track, obs in tracks_manager.get_shot_observations(shot_id).items():
        if track in reconstruction.points:
            xy.append(obs.point)
            Xs.append(reconstruction.points[track].coordinates)
            ids.append(track)
    if len(xy) < 5:
        return False, set(), {"num_common_points": len(xy)}
    bs = matching.pixel_bearing_many(camera, np.array(xy), gpu_ctx)
    Xs = np.array(Xs)
    res, _, cmask = host_images(host, bs, Xs, [0, len(bs)], threshold)
    Rt = np.array(res[0].lo_model).reshape(3, 4)
    R, t = Rt[:3, :3].copy(), Rt[:, 3].copy()
    T = Rt.copy()
    T[:3, :3] = R.T
    T[:, 3] = -R.T.dot(t)
    inliers = cmask
    ninliers = int(sum(inliers))
    report = {"num_common_points": len(bs), "num_inliers": ninliers}
    if ninliers < min_inliers:
        return False, set(), report
    R = T[:, :3].T
    t = -R.dot(T[:, 3])
    pose = Pose(translation=t)
    pose.set_rotation_matrix(R)
    if shot_id not in rig_assignments:
        reconstruction.create_shot(shot_id, data.load_exif(shot_id)["camera"], pose)
        new_shots = {shot_id}
    else:
        instance_id, _, instance_shots = rig_assignments[shot_id]
        rig_instance = reconstruction.add_rig_instance(RigInstance(instance_id))
        for shot in instance_shots:
            reconstruction.create_shot(shot, data.load_exif(shot)["camera"], Pose(), rig_assignments[shot][1], instance_id)
        rig_instance.pose = reconstruction.shots[shot_id].rig_camera.pose.inverse().compose(pose)
        new_shots = set(instance_shots)
        rec_mod.triangulate_shot_features(tracks_manager, reconstruction, new_shots, data.config, ctx=gpu_ctx)
    for i, succeed in enumerate(inliers):
        if succeed:
            reconstruction.add_observation(shot_id, ids[i], tracks_manager.get_observation(shot_id, ids[i]))
    report["shots"] = list(new_shots)
    return True, new_shots, report


def _same_map(a, b):
    assert list(a.shots) == list(b.shots)
    for s in a.shots:
        assert same_bits(a.shots[s].pose.rotation, b.shots[s].pose.rotation) and same_bits(a.shots[s].pose.translation, b.shots[s].pose.translation), s
        assert list(a.shots[s].observations) == list(b.shots[s].observations), s
    assert list(a.points) == list(b.points)
    for p in a.points:
        assert same_bits(a.points[p].coordinates, b.points[p].coordinates), p


def _same_report(a, b):
    assert {k: (sorted(v) if k == "shots" else v) for k, v in a.items()} == {k: (sorted(v) if k == "shots" else v) for k, v in b.items()}


@pytest.fixture(scope="module")
def scene():
    from opensfm_amd import synthetic

    return synthetic.make_resection_scene()


def test_resect_equals_host_loop(host, scene, gpu_ctx):
    from opensfm_amd import reconstruction

    data, tm, rec0, truth = scene
    threshold, min_inliers = data.config["resection_threshold"], data.config["resection_min_inliers"]
    outcomes = {}
    for image in ("held_few_points", "held_few_inliers", "held_ok", "rig_b"):
        got_rec, want_rec = copy.deepcopy(rec0), copy.deepcopy(rec0)
        ok, new_shots, report = reconstruction.resect(data, tm, got_rec, image, threshold, min_inliers, ctx=gpu_ctx)
        wok, wnew, wreport = _host_resect(host, data, tm, want_rec, image, threshold, min_inliers, gpu_ctx)
        assert (ok, new_shots) == (wok, wnew), image
        _same_report(report, wreport)
        _same_map(got_rec, want_rec)
        outcomes[image] = (ok, report, got_rec)
    assert outcomes["held_few_points"][:2] == (False, {"num_common_points": 4})
    ok, report, _ = outcomes["held_few_inliers"]
    assert not ok and report["num_common_points"] == 40 and report["num_inliers"] < min_inliers
    ok, report, rec = outcomes["held_ok"]
    assert ok and report["num_common_points"] == 300 and report["num_inliers"] > 200 and report["shots"] == ["held_ok"]
    R, t = truth["held_ok"]
    assert np.abs(rec.shots["held_ok"].pose.get_rotation_matrix() - R).max() < 1e-3 and np.abs(rec.shots["held_ok"].pose.translation - t).max() < 1e-2
    assert len(rec.shots["held_ok"].observations) == report["num_inliers"]
    ok, report, rec = outcomes["rig_b"]  # a rig-assigned image adds its whole instance, posed through its rig camera, and triangulates
    assert ok and sorted(report["shots"]) == ["rig_a", "rig_b"]
    for image in ("rig_a", "rig_b"):
        R, t = truth[image]
        assert np.abs(rec.shots[image].pose.get_rotation_matrix() - R).max() < 1e-3 and np.abs(rec.shots[image].pose.translation - t).max() < 1e-2
    assert len(rec.points) > len(rec0.points) + 40


def test_resect_candidates_equals_host_loop(host, scene, gpu_ctx):
    from opensfm_amd import reconstruction

    data, tm, rec0, _ = scene
    threshold, min_inliers = data.config["resection_threshold"], data.config["resection_min_inliers"]
    candidates = reconstruction.reconstructed_points_for_images(tm, rec0, ["held_few_points", "held_few_inliers", "held_ok", "rig_a", "im00"])
    assert candidates == [("held_ok", 300), ("rig_a", 200), ("held_few_inliers", 40), ("held_few_points", 4)]
    for order, max_batch in ((candidates[::-1], 8), (candidates[::-1], 2), (candidates[::-1], 1), (candidates, 8), (candidates[2:], 8)):
        got_rec, want_rec = copy.deepcopy(rec0), copy.deepcopy(rec0)
        got = reconstruction.resect_candidates(data, tm, got_rec, order, threshold, min_inliers, max_batch=max_batch, ctx=gpu_ctx)
        added, failed = None, []
        for image, _ in order:  # grow_reconstruction's loop up to the first success
            ok, new_shots, report = _host_resect(host, data, tm, want_rec, image, threshold, min_inliers, gpu_ctx)
            if ok:
                added = (image, new_shots, report)
                break
            failed.append((image, report))
        assert [f[0] for f in got["failed"]] == [f[0] for f in failed]
        for g, w in zip(got["failed"], failed):
            _same_report(g[1], w[1])
        if added is None:
            assert got["image"] is None and got["new_shots"] == set() and got["report"] is None
        else:
            assert (got["image"], got["new_shots"]) == added[:2]
            _same_report(got["report"], added[2])
        _same_map(got_rec, want_rec)
    assert added is None and len(failed) == 2  # the last order holds the two images that cannot be resected


def test_documented_errors(gpu_ctx):
    from opensfm_amd import reconstruction
    from opensfm_amd._lib import OsfmError
    from opensfm_amd.compat import pygeometry, pyrobust

    res, rmask, cmask, ms = reconstruction.abspose_images(np.zeros((0, 3)), np.zeros((0, 3)), [0], THRESHOLD, ctx=gpu_ctx)  # empty batch: nothing
    assert res == [] and len(rmask) == 0 and len(cmask) == 0 and ms == 0.0
    b = np.tile(np.array([[0.0, 0.0, 1.0]]), (10, 1))
    for off in ([0, 0, 10], [0, 2, 10], [0, 8, 10]):  # zero-length image, n < 3 first / last
        with pytest.raises(OsfmError, match="at least 3"):
            reconstruction.abspose_images(b, b, off, THRESHOLD, ctx=gpu_ctx)
    for args in ((b, b[:9], [0, 10]), (b, b, [0, 5, 9])):  # mismatched lengths
        with pytest.raises(ValueError):
            reconstruction.abspose_images(*args, THRESHOLD, ctx=gpu_ctx)
    with pytest.raises(RuntimeError):
        pyrobust.ransac_absolute_pose(b[:2], b[:2], 0.01, pyrobust.RobustEstimatorParams())
    with pytest.raises(RuntimeError, match="different sizes"):
        pyrobust.ransac_absolute_pose(b[:5], b[:4], 0.01, pyrobust.RobustEstimatorParams())
    xy = np.zeros((10, 2))
    for ic, cm, cp in ((np.zeros(1), [0], np.zeros((1, 16))), (np.zeros(2), [0, 0], np.zeros((1, 16))), (np.zeros(2), [0], np.zeros((1, 9)))):
        with pytest.raises(ValueError):  # image_cam / camera table of the wrong shape: refused before the call
            reconstruction.abspose_images_pixels(xy, b, [0, 5, 10], ic, cm, cp, THRESHOLD, ctx=gpu_ctx)
    for ic, image in (([0, 1], 1), ([-1, 0], 0)):  # a camera index outside the table
        with pytest.raises(OsfmError, match=re.escape("(-1): osfm_abspose_images_pixels: image %d names a camera outside the table" % image) + "$"):
            reconstruction.abspose_images_pixels(xy, b, [0, 5, 10], np.array(ic), [0], np.zeros((1, 16)), THRESHOLD, ctx=gpu_ctx)
    with pytest.raises(OsfmError, match="at least 3"):
        pygeometry.absolute_pose_n_points(b[:2], b[:2])
    prm = pyrobust.RobustEstimatorParams()
    with pytest.raises(NotImplementedError):
        pyrobust.ransac_absolute_pose(b, b, 0.01, prm, pyrobust.MSAC)
    with pytest.raises(NotImplementedError):
        pyrobust.ransac_absolute_pose(b, b, 0.01, prm, pyrobust.LMedS)
    prm.use_iteration_reduction = False
    with pytest.raises(NotImplementedError):
        pyrobust.ransac_absolute_pose(b, b, 0.01, prm)
    with pytest.raises(ValueError):
        reconstruction.resect_candidates(None, None, None, [], THRESHOLD, 10, max_batch=0)
