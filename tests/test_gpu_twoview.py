"""osfm_two_view_pairs on the MI355X against the host build of the same header (tests/native/twoview_host.cpp, itself held bit for bit to
the oracle's leaves by tests/test_twoview_host.py): statuses, chosen configurations and all three mask bits identical, the RANSAC's
score / iterations / lo_model bit-equal (as tests/test_gpu_zz_relpose.py requires of the same rounds), the refined R / t within 1e-6 (the
bound that file uses for this refinement: the device's sin / cos differ from the host's in the last bits).  Also: batch independence,
the pixels twin, the drop-ins with the reference's signatures, and the documented errors."""
import ctypes as C

import numpy as np
import pytest

import twoview_cases as cases
from test_gpu_relrot import _Cam, _project

pytestmark = pytest.mark.gpu

POSE_BOUND = 1e-6
FIELDS = ("status", "chosen", "R", "t", "n_inliers", "refine_iterations", "rotation", "translation", "lo_model", "score", "iterations")


@pytest.fixture(scope="module")
def host():
    return cases.build_host()


@pytest.fixture(scope="module")
def ransac_batch(host):
    """the RANSAC cases as one ragged batch, with the host build's results: computed once, shared, left unchanged"""
    group = cases.ransac_cases()
    b1, b2, off, _ = cases.batch(group)
    want, wmask = cases.host_pairs(host, b1, b2, off, None, cases.THRESHOLD, True, 0.95)
    return group, b1, b2, off, want, wmask


def _same_as_host(got, mask, want, wmask, names, ransac):
    seen = set()
    for g, w, name in zip(got, want, names):
        assert (g["status"], g["chosen"]) == (w.status, w.chosen), name
        assert g["n_inliers"] == list(w.n_inliers), name
        seen.add(cases.outcome(w.status, w.chosen, w.n_inliers[0], w.n_inliers[1]))
        if ransac:
            assert (g["score"], g["iterations"]) == (w.score, w.iterations), name
            assert g["lo_model"].tobytes() == np.array(w.lo_model).tobytes(), name
        else:
            assert g["score"] == 0 and g["iterations"] == 0 and not g["lo_model"].any(), name
        for c in range(2):
            if w.n_inliers[c] < 0:
                assert not g["R"][c].any() and not g["t"][c].any(), name
                continue
            dR = np.abs(g["R"][c].ravel() - np.array(w.R[9 * c: 9 * c + 9])).max()
            dt = np.abs(g["t"][c] - np.array(w.t[3 * c: 3 * c + 3])).max()
            assert dR < POSE_BOUND and dt < POSE_BOUND, (name, c, dR, dt)
        if w.status == cases.OK:
            assert np.abs(g["rotation"] - np.array(w.rotation)).max() < POSE_BOUND and np.abs(g["translation"] - np.array(w.translation)).max() < POSE_BOUND
        else:
            assert not g["rotation"].any() and not g["translation"].any(), name
    assert np.array_equal(mask, wmask)
    return seen


def test_ransac_batch_equals_host_build(ransac_batch, gpu_ctx):
    from opensfm_amd import reconstruction

    group, b1, b2, off, want, wmask = ransac_batch
    got, mask, ms = reconstruction.two_view_pairs(b1, b2, off, cases.THRESHOLD, check_reversal=True, reversal_ratio=0.95, ctx=gpu_ctx)
    assert len(got) == len(group) and ms > 0
    seen = _same_as_host(got, mask, want, wmask, [c.name for c in group], True)
    assert {"OK-0", "none"} <= seen, seen


def test_given_pose_cases_equal_host_build(host, gpu_ctx):
    from opensfm_amd import reconstruction

    seen, pairs = set(), 0
    for (threshold, check_reversal, ratio), group in cases.by_params(cases.given_pose_cases()).items():
        b1, b2, off, poses = cases.batch(group)
        want, wmask = cases.host_pairs(host, b1, b2, off, poses, threshold, check_reversal, ratio)
        got, mask, _ = reconstruction.two_view_pairs(b1, b2, off, threshold, poses=poses, check_reversal=check_reversal, reversal_ratio=ratio,
                                                     ctx=gpu_ctx)
        for c, g in zip(group, got):
            assert (g["status"], g["chosen"]) == c.expect, c.name
        seen |= _same_as_host(got, mask, want, wmask, [c.name for c in group], False)
        pairs += len(got)
    assert seen == cases.OUTCOMES, seen  # no branch passes by never being taken
    assert pairs == len(cases.given_pose_cases())  # and no pair is skipped


def test_batch_equals_single_pair_calls(ransac_batch, gpu_ctx):
    from opensfm_amd import reconstruction

    group, b1, b2, off, _, _ = ransac_batch
    got, mask, _ = reconstruction.two_view_pairs(b1, b2, off, cases.THRESHOLD, check_reversal=True, reversal_ratio=0.95, ctx=gpu_ctx)
    for k, c in enumerate(group):
        one, one_mask, _ = reconstruction.two_view_pairs(c.b1, c.b2, [0, len(c.b1)], cases.THRESHOLD, check_reversal=True, reversal_ratio=0.95,
                                                         ctx=gpu_ctx)
        for f in FIELDS:
            assert np.asarray(one[0][f]).tobytes() == np.asarray(got[k][f]).tobytes(), (c.name, f)
        assert one_mask.tobytes() == mask[off[k]: off[k + 1]].tobytes(), c.name


def _pixel_pairs():
    persp = _Cam("perspective", focal=0.9, k1=-0.05, k2=0.01)
    brown = _Cam("brown", focal=0.85, aspect_ratio=1.02, k1=-0.03, k2=0.005, k3=0.0, p1=1e-3, p2=-5e-4, principal_point=(0.01, -0.02))
    pairs = []
    for k, (n, cam1, cam2) in enumerate(((120, persp, brown), (5, brown, brown), (65, brown, persp))):
        b1, b2, _, _ = cases.scene(np.random.default_rng(600 + k), n)
        assert (b1[:, 2] > 0.5).all() and (b2[:, 2] > 0.5).all()  # in front of both cameras
        pairs.append((_project(cam1, b1), _project(cam2, b2), cam1, cam2))
    return pairs


def test_pixels_twin_equals_bearings_call(gpu_ctx):
    from opensfm_amd import matching, reconstruction

    pairs = _pixel_pairs()
    cams = [pairs[0][2], pairs[0][3]]  # perspective, Brown: one table
    models, params = zip(*(matching.camera_parameters(c) for c in cams))
    pair_cams = np.array([[cams.index(p[2]), cams.index(p[3])] for p in pairs], np.int32)
    off = np.r_[0, np.cumsum([len(p[0]) for p in pairs])].astype(np.int64)
    got, mask, _ = reconstruction.two_view_pairs_pixels(np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs]), off, pair_cams,
                                                        np.array(models, np.int32), np.array(params), cases.THRESHOLD, check_reversal=True,
                                                        reversal_ratio=0.95, ctx=gpu_ctx)
    b1 = np.concatenate([matching.pixel_bearing_many(p[2], p[0], gpu_ctx) for p in pairs])
    b2 = np.concatenate([matching.pixel_bearing_many(p[3], p[1], gpu_ctx) for p in pairs])
    want, wmask, _ = reconstruction.two_view_pairs(b1, b2, off, cases.THRESHOLD, check_reversal=True, reversal_ratio=0.95, ctx=gpu_ctx)
    for g, w in zip(got, want):
        for f in FIELDS:
            assert np.asarray(g[f]).tobytes() == np.asarray(w[f]).tobytes(), f
    assert mask.tobytes() == wmask.tobytes()
    assert [g["status"] for g in got] == [cases.OK, cases.NO_CONFIGURATION, cases.OK]


def test_five_point_drop_ins_return_the_reference_tuples(host, gpu_ctx):
    from opensfm_amd import reconstruction

    by_name = {c.name: c for c in cases.given_pose_cases()}
    c = by_name["symmetric pose, ratio 0.95"]
    assert reconstruction.two_view_reconstruction_5pt(c.b1, c.b2, c.pose[0], c.pose[1], c.threshold, 1000, True, 0.95, ctx=gpu_ctx) == (None, None, [])
    R, t, inliers = reconstruction.two_view_reconstruction_5pt(c.b1, c.b2, c.pose[0], c.pose[1], c.threshold, 1000, True, 1.0, ctx=gpu_ctx)
    want, wmask = cases.host_pairs(host, c.b1, c.b2, [0, len(c.b1)], np.r_[c.pose[0].ravel(), c.pose[1]], c.threshold, True, 1.0)
    assert want[0].chosen == 1 and np.array_equal(inliers, np.flatnonzero(wmask >> 2 & 1))
    assert np.abs(R - np.array(want[0].rotation)).max() < POSE_BOUND and np.abs(t - np.array(want[0].translation)).max() < POSE_BOUND
    c = by_name["true pose n=5"]
    assert reconstruction.two_view_reconstruction_5pt(c.b1, c.b2, c.pose[0], c.pose[1], c.threshold, 1000, ctx=gpu_ctx) == (None, None, [])
    # one configuration on its own, the given and the transposed pose
    c = by_name["inverse pose n=65"]
    want, wmask = cases.host_pairs(host, c.b1, c.b2, [0, 65], np.r_[c.pose[0].ravel(), c.pose[1]], c.threshold, True, 0.95)
    for transposed in (False, True):
        R, t, inliers = reconstruction.two_view_reconstruction_and_refinement(c.b1, c.b2, c.pose[0], c.pose[1], c.threshold, 1000, transposed, ctx=gpu_ctx)
        k = int(transposed)
        assert np.array_equal(inliers, np.flatnonzero(wmask >> k & 1))
        assert np.abs(t - np.array(want[0].t[3 * k: 3 * k + 3])).max() < POSE_BOUND
        back = np.zeros(9)
        host.host_aa_to_rotmat(np.ascontiguousarray(R).ctypes.data_as(C.POINTER(C.c_double)), back.ctypes.data_as(C.POINTER(C.c_double)))
        assert np.abs(back - np.array(want[0].R[9 * k: 9 * k + 9])).max() < POSE_BOUND


def test_general_drop_in_with_and_without_a_plane_branch(gpu_ctx):
    from opensfm_amd import reconstruction

    pairs = _pixel_pairs()
    p1, p2, cam1, cam2 = pairs[0]
    R, t, inliers, report = reconstruction.two_view_reconstruction_general(p1, p2, cam1, cam2, cases.THRESHOLD, 1000, True, 0.95, ctx=gpu_ctx)
    assert report == {"5_point_inliers": len(inliers), "plane_based_inliers": 0, "method": "5_point"} and len(inliers) > 60
    assert R.shape == (3,) and t.shape == (3,)
    seen = []

    def plane_based(b1, b2, threshold):  # a plane branch that claims every correspondence
        seen.append((b1.shape, b2.shape, threshold))
        return np.zeros(3), np.array([1.0, 0.0, 0.0]), np.arange(len(b1))

    R2, t2, inliers2, report2 = reconstruction.two_view_reconstruction_general(p1, p2, cam1, cam2, cases.THRESHOLD, 1000, True, 0.95,
                                                                               plane_based=plane_based, ctx=gpu_ctx)
    assert report2 == {"5_point_inliers": len(inliers), "plane_based_inliers": len(p1), "method": "plane_based"}
    assert seen == [((len(p1), 3), (len(p1), 3), cases.THRESHOLD)] and len(inliers2) == len(p1) and not R2.any()
    # the batch form: the look-ahead over several ranked pairs, the small pair included
    out = reconstruction.two_view_reconstruction_general_pairs(pairs, cases.THRESHOLD, 1000, True, 0.95, ctx=gpu_ctx)
    assert [r[3].get("method") for r in out] == ["5_point", None, "5_point"]
    assert out[1][:3] == (None, None, []) and out[1][3]["decision"] == "Could not find initial motion"
    assert np.array_equal(out[0][0], R) and np.array_equal(out[0][2], inliers)


def test_relative_pose_refinement_leaf_against_the_oracle(gpu_ctx):
    import oracle
    from opensfm_amd.compat import pygeometry

    b1, b2, R, t = cases.scene(np.random.default_rng(7), 101, outliers=0.0)
    noisy = cases.rodrigues(np.array([0.01, -0.02, 0.015])) @ R
    start = np.c_[noisy, t]
    want, its, _ = oracle.relative_pose_refinement(start, b1, b2, 20)
    got = pygeometry.relative_pose_refinement(start, b1, b2, 20)
    assert its > 1 and np.abs(want - start).max() > 1e-4  # the refinement moved the pose
    assert got.shape == (3, 4) and np.abs(got - want).max() < POSE_BOUND


def test_documented_errors(gpu_ctx):
    from opensfm_amd import _lib

    lib = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    prm = _lib.TwoViewParams(0.004, 0.99, 1.0, 1000, 1, 10, 1000, 0, 0)
    b = np.zeros((12, 3))
    res = (_lib.TwoViewResult * 2)()
    mask = np.zeros(12, np.uint8)
    args = lambda off, n, b1=b: (gpu_ctx.handle, None if b1 is None else b1.ctypes.data_as(dp), b.ctypes.data_as(dp),  # noqa: E731
                                 np.asarray(off, np.int64).ctypes.data_as(C.POINTER(C.c_int64)), n)
    tail = (None, C.byref(prm), res, mask.ctypes.data_as(C.POINTER(C.c_uint8)), None)
    assert lib.osfm_two_view_pairs(*args([0, 6, 12], -1), *tail) == -1  # n_pairs < 0
    assert lib.osfm_two_view_pairs(*args([0, 8, 6], 2), *tail) == -1  # descending offsets
    assert lib.osfm_two_view_pairs(*args([0, 6, 12], 2, None), *tail) == -1  # null bearings
    assert b"null" in lib.osfm_last_error()
    assert lib.osfm_two_view_pairs(*args([0], 0), *tail) == 0  # nothing to do
    pc, cm, cp = np.array([[0, 0], [0, 1]], np.int32), np.zeros(1, np.int32), np.zeros((1, 16))
    p = np.zeros((12, 2))
    assert lib.osfm_two_view_pairs_pixels(gpu_ctx.handle, p.ctypes.data_as(dp), p.ctypes.data_as(dp),
                                          np.array([0, 6, 12], np.int64).ctypes.data_as(C.POINTER(C.c_int64)), 2, pc.ctypes.data_as(ip),
                                          cm.ctypes.data_as(ip), cp.ctypes.data_as(dp), 1, *tail) == -1  # pair 1 names camera 1 of a table of 1
    assert b"camera" in lib.osfm_last_error()
