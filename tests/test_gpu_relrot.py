"""Rotation-only LO-RANSAC of compute_image_pairs on the MI355X (relrot.hip): every result field and the inlier mask equal to the host
build of the same header (tests/native/relrot_host.cpp) bit for bit; the documented errors; compat.pyrobust.ransac_relative_rotation
against the reference test's tolerances; opensfm_amd.reconstruction.compute_image_pairs against the host restatement of the
reference's flow on a fake DataSet with four camera models."""

import re

import numpy as np
import pytest

from test_relrot_host import build_host, host_pairs, make_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return build_host()


def _batch(seed=0, count=2000):
    rng = np.random.default_rng(seed)
    probs = []
    for k in range(count):
        if k == 0:
            n = 20000  # longer than the LDS inlier list: the scratch path
        elif k < 12:
            n = 3 + k
        else:
            n = int(np.exp(rng.uniform(np.log(3), np.log(2500))))
        kind = k % 4
        if kind == 0:
            probs.append(make_problem(rng, n, outliers=rng.uniform(0, 0.4)))
        elif kind == 1:
            probs.append(make_problem(rng, n, outliers=rng.uniform(0, 0.8), baseline=rng.uniform(0.1, 1.5)))
        elif kind == 2:
            probs.append(make_problem(rng, n, outliers=0.0, exact=True))
        else:
            probs.append(make_problem(rng, n, outliers=rng.uniform(0.2, 0.9), duplicates=max(1, n // 10)))
    b1 = np.concatenate([p[0] for p in probs])
    b2 = np.concatenate([p[1] for p in probs])
    off = np.r_[0, np.cumsum([len(p[0]) for p in probs])].astype(np.int64)
    return b1, b2, off


def test_batch_equals_host_build_bit_for_bit(host, gpu_ctx):
    from opensfm_amd import reconstruction

    b1, b2, off = _batch()
    assert (np.diff(off) > 4096).any()
    got, mask, ms = reconstruction.relrot_pairs(b1, b2, off, 0.016, inlier_chord=0.016, ctx=gpu_ctx)
    want, wmask = host_pairs(host, b1, b2, off, 0.016, chord=0.016)
    assert ms > 0
    for p, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["model"].ravel(), np.array(w.model)), p
        assert np.array_equal(g["lo_model"].ravel(), np.array(w.lo_model)), p
        assert (g["score"], g["iterations"], g["n_rotation_inliers"], g["reconstructability"]) == \
            (w.score, w.iterations, w.n_rotation_inliers, w.reconstructability), p
    assert np.array_equal(mask, wmask)
    assert sum(g["reconstructability"] > 0 for g in got) > 100 and sum(g["reconstructability"] == 0 for g in got) > 100


def test_parameters_without_lo_and_reduction_equal_host(host, gpu_ctx):
    from opensfm_amd import reconstruction

    b1, b2, off = _batch(seed=1, count=200)
    got, mask, _ = reconstruction.relrot_pairs(b1, b2, off, 0.01, iterations=120, use_lo=False, use_iteration_reduction=False, ctx=gpu_ctx)
    want, wmask = host_pairs(host, b1, b2, off, 0.01, iterations=120, use_lo=0, use_reduction=0)
    for g, w in zip(got, want):
        assert np.array_equal(g["lo_model"].ravel(), np.array(w.lo_model)) and (g["score"], g["iterations"]) == (w.score, w.iterations)
        assert g["n_rotation_inliers"] == -1
    assert np.array_equal(mask, wmask)


def test_documented_errors(gpu_ctx):
    from opensfm_amd import reconstruction
    from opensfm_amd._lib import OsfmError
    from opensfm_amd.compat import pyrobust

    res, mask, ms = reconstruction.relrot_pairs(np.zeros((0, 3)), np.zeros((0, 3)), [0], 0.016, ctx=gpu_ctx)  # empty batch: nothing
    assert res == [] and len(mask) == 0 and ms == 0.0
    b = np.tile(np.array([[0.0, 0.0, 1.0]]), (10, 1))
    for off in ([0, 0, 10], [0, 2, 10], [0, 8, 10]):  # zero-length pair, N < 3 first / last
        with pytest.raises(OsfmError, match="at least 3"):
            reconstruction.relrot_pairs(b, b, off, 0.016, ctx=gpu_ctx)
    with pytest.raises(RuntimeError):
        pyrobust.ransac_relative_rotation(b[:2], b[:2], 0.01, pyrobust.RobustEstimatorParams())
    with pytest.raises(RuntimeError, match="different sizes"):
        pyrobust.ransac_relative_rotation(b[:5], b[:4], 0.01, pyrobust.RobustEstimatorParams())
    px = np.zeros((10, 2))
    for pc, cm, cp in ((np.zeros((1, 2)), [0], np.zeros((1, 16))), (np.zeros((2, 2)), [0, 0], np.zeros((1, 16))),
                       (np.zeros((2, 2)), [0], np.zeros((1, 9)))):  # pair_cams / camera table of the wrong shape: refused before the call
        with pytest.raises(ValueError):
            reconstruction.relrot_pairs_pixels(px, px, [0, 5, 10], pc, cm, cp, 0.016, ctx=gpu_ctx)
    # one pair of 3 correspondences with a bad camera table: refused before any kernel is launched
    with pytest.raises(OsfmError, match=re.escape("(-1): osfm_relrot_pairs_pixels: camera 0 has model 99") + "$"):
        reconstruction.relrot_pairs_pixels(px[:3], px[:3], [0, 3], np.array([[0, 0]]), [99], np.zeros((1, 16)), 0.016, ctx=gpu_ctx)
    with pytest.raises(OsfmError, match=re.escape("(-1): osfm_relrot_pairs_pixels: pair 0 names a camera outside the table") + "$"):
        reconstruction.relrot_pairs_pixels(px[:3], px[:3], [0, 3], np.array([[0, -1]]), [0], np.zeros((1, 16)), 0.016, ctx=gpu_ctx)
    prm = pyrobust.RobustEstimatorParams()
    with pytest.raises(NotImplementedError):
        pyrobust.ransac_relative_rotation(b, b, 0.01, prm, pyrobust.MSAC)
    prm.use_iteration_reduction = False
    with pytest.raises(NotImplementedError):
        pyrobust.ransac_relative_rotation(b, b, 0.01, prm)


def test_pyrobust_relative_rotation_reference_tolerances(gpu_ctx):
    """test_robust.py::test_outliers_relative_rotation_ransac restaged with this repo's data: inliers within 4 %, Frobenius < 8e-2"""
    from opensfm_amd.compat import pyrobust

    rng = np.random.default_rng(21)
    for _ in range(6):
        f1 = np.c_[rng.uniform(-2, 2, 400), rng.uniform(-2, 2, 400), rng.uniform(4, 9, 400)]
        vec_x = rng.random(3)
        vec_x /= np.linalg.norm(vec_x)
        vec_y = np.array([-vec_x[1], vec_x[0], 0.0])
        vec_y /= np.linalg.norm(vec_y)
        rotation = np.array([vec_x, vec_y, np.cross(vec_x, vec_y)])
        f1 /= np.linalg.norm(f1, axis=1)[:, None]
        points = np.concatenate((f1, f1 @ rotation.T), axis=1)
        scale = 1e-3
        points += rng.random(points.shape) * scale
        ratio_outliers = 0.3
        bad = rng.choice(len(points), int(ratio_outliers * len(points)), replace=False)
        points[bad] += rng.uniform(0.1, 1.0, (len(bad), 6)) * rng.choice([-1, 1], (len(bad), 6))
        a, b = points[:, :3], points[:, 3:]
        a /= np.linalg.norm(a, axis=1)[:, None]
        b /= np.linalg.norm(b, axis=1)[:, None]
        params = pyrobust.RobustEstimatorParams()
        params.iterations = 1000
        result = pyrobust.ransac_relative_rotation(a, b, np.sqrt(3 * scale * scale), params, pyrobust.RansacType.RANSAC)
        assert np.isclose(len(result.inliers_indices), (1 - ratio_outliers) * len(points), rtol=0.04)
        assert np.linalg.norm(rotation - result.lo_model, ord="fro") < 8e-2


class _Cam:
    def __init__(self, projection_type, **kw):
        self.projection_type = projection_type
        self.principal_point = kw.pop("principal_point", (0.0, 0.0))
        for k, v in kw.items():
            setattr(self, k, v)


class _FakeData:
    """the three things compute_image_pairs reads from a DataSet"""

    def __init__(self, cameras, image_camera):
        self.config = {"five_point_algo_threshold": 0.004, "processes": 1}
        self._cameras, self._image_camera = cameras, image_camera

    def load_camera_models(self):
        return self._cameras

    def load_exif(self, im):
        return {"camera": self._image_camera[im]}


def _project(cam, b):
    """normalised image coordinates of unit bearings (camera z > 0) for the four models used here (inverse of pixel_bearing_many)"""
    x, y, z = b[:, 0], b[:, 1], b[:, 2]
    if cam.projection_type == "spherical":
        lon = np.arctan2(x, z)
        lat = np.arctan2(-y, np.sqrt(x * x + z * z))
        return np.c_[lon / (2 * np.pi), -lat / (2 * np.pi)]
    if cam.projection_type == "fisheye":
        r = np.sqrt(x * x + y * y)
        th = np.arctan2(r, z)
        d = 1 + cam.k1 * th**2 + cam.k2 * th**4
        s = np.where(r > 0, cam.focal * d * th / np.maximum(r, 1e-300), 0.0)
        return np.c_[s * x, s * y]
    xn, yn = x / z, y / z
    if cam.projection_type == "brown":
        r2 = xn * xn + yn * yn
        d = 1 + cam.k1 * r2 + cam.k2 * r2**2 + cam.k3 * r2**3
        xd = xn * d + 2 * cam.p1 * xn * yn + cam.p2 * (r2 + 2 * xn * xn)
        yd = yn * d + cam.p1 * (r2 + 2 * yn * yn) + 2 * cam.p2 * xn * yn
        return np.c_[cam.focal * xd + cam.principal_point[0], cam.focal * cam.aspect_ratio * yd + cam.principal_point[1]]
    r2 = xn * xn + yn * yn
    d = 1 + cam.k1 * r2 + cam.k2 * r2**2
    return np.c_[cam.focal * d * xn, cam.focal * d * yn]


def _scene(seed=3, n_images=12):
    rng = np.random.default_rng(seed)
    cameras = {
        "persp": _Cam("perspective", focal=0.9, k1=-0.05, k2=0.01),
        "brown": _Cam("brown", focal=0.85, aspect_ratio=1.02, k1=-0.03, k2=0.005, k3=0.0, p1=1e-3, p2=-5e-4, principal_point=(0.01, -0.02)),
        "fish": _Cam("fisheye", focal=0.6, k1=-0.02, k2=0.003),
        "sph": _Cam("spherical"),
    }
    keys = list(cameras)
    images = ["im%02d" % i for i in range(n_images)]
    image_camera = {im: keys[i % 4] for i, im in enumerate(images)}
    track_dict = {}
    for i in range(n_images):
        for j in range(i + 1, n_images):
            if rng.random() < 0.45:
                continue
            n = int(rng.integers(50, 1200))
            b1, b2 = make_problem(rng, n, outliers=rng.uniform(0.0, 0.6), noise=1e-3, baseline=rng.choice([0.0, 0.0, 0.3, 1.0]))
            b1[:, 2], b2[:, 2] = np.abs(b1[:, 2]), np.abs(b2[:, 2])  # in front of both cameras
            p1 = _project(cameras[image_camera[images[i]]], b1)
            p2 = _project(cameras[image_camera[images[j]]], b2)
            track_dict[(images[i], images[j])] = (np.arange(n), p1, p2)
    return track_dict, _FakeData(cameras, image_camera)


def test_compute_image_pairs_equals_host_restatement(host, gpu_ctx):
    """the drop-in against the reference's flow restated on the host (bearings from the GPU's pixel_bearing_many, the estimator of
    the host build, _two_view_rotation_inliers in numpy, pairwise_reconstructability, argsort); correspondences within a few ulp of the
    chord are counted and may fall either way (numpy's R.dot goes through BLAS)"""
    from opensfm_amd import matching, reconstruction

    track_dict, data = _scene()
    cameras = data.load_camera_models()
    threshold = 4 * data.config["five_point_algo_threshold"]
    pairs, score, borderline, slack = [], [], 0, {}
    for (im1, im2), (_, p1, p2) in track_dict.items():
        b1 = matching.pixel_bearing_many(cameras[data.load_exif(im1)["camera"]], p1, gpu_ctx)
        b2 = matching.pixel_bearing_many(cameras[data.load_exif(im2)["camera"]], p2, gpu_ctx)
        res, _ = host_pairs(host, b1, b2, [0, len(b1)], threshold)
        R = np.array(res[0].lo_model).reshape(3, 3).T
        d = np.linalg.norm(R.dot(b2.T).T - b1, axis=1)
        near = np.abs(d - threshold) <= 8 * np.spacing(threshold)
        borderline += int(near.sum())
        r = reconstruction.pairwise_reconstructability(len(p1), int((d < threshold).sum()))
        if near.any():
            slack[(im1, im2)] = int(near.sum())
        if r > 0:
            pairs.append((im1, im2))
            score.append(r)
    want = [pairs[o] for o in np.argsort(-np.array(score))]
    got = reconstruction.compute_image_pairs(track_dict, data, ctx=gpu_ctx)
    assert len(want) > 10 and len(track_dict) - len(want) >= 1
    if not slack:
        assert got == want
    else:  # only the pairs with a borderline row may move; every other pair keeps its place relative to the others
        stable = lambda lst: [p for p in lst if p not in slack]  # noqa: E731
        assert stable(got) == stable(want), borderline
    assert borderline <= 2


def test_pyrobust_local_optimization_iterations_reach_both_estimators(gpu_ctx):
    """RobustEstimatorParams.local_optimization_iterations is honoured by ransac_relative_rotation and ransac_relative_pose alike"""
    from opensfm_amd import matching, reconstruction
    from opensfm_amd.compat import pyrobust

    rng = np.random.default_rng(8)
    b1, b2 = make_problem(rng, 300, outliers=0.4)
    prm = pyrobust.RobustEstimatorParams()
    prm.iterations = 200
    prm.local_optimization_iterations = 3
    rot = pyrobust.ransac_relative_rotation(b1, b2, 0.01, prm)
    want, _, _ = reconstruction.relrot_pairs(b1, b2, [0, len(b1)], 0.01, iterations=200, lo_iterations=3, ctx=gpu_ctx)
    assert np.array_equal(rot.lo_model, want[0]["lo_model"]) and rot.score == want[0]["score"]
    pose = pyrobust.ransac_relative_pose(b1, b2, 0.004, prm)
    want, _, _ = matching.relpose_pairs(b1, b2, [0, len(b1)], 0.004, mode="ransac", iterations=200, lo_iterations=3, ctx=gpu_ctx)
    assert np.array_equal(pose.lo_model, want[0]["lo_model"]) and pose.score == want[0]["score"]
