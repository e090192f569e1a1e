"""osfm_two_view_plane_pairs on the MI355X against the host build of the same header (tests/native/plane_host.cpp, itself held to the
numpy restatement by tests/test_plane_host.py): status, h_inliers, iterations, motion_inliers, chosen, both mask bits, H, singular, R
and t bit for bit (the arithmetic is + - * / sqrt under -ffp-contract=off); the angle-axis through its rotation matrix (the device's
atan2 differs from the host's in the last bits).  Also: the leaf entries against the restatement, the pixels twin, batch independence,
refusals that leave the outputs untouched, the "device" plane branch of two_view_reconstruction_general_pairs and the drop-ins."""
import ctypes as C

import numpy as np
import pytest

import plane_cases as cases
from test_gpu_relrot import _Cam, _project
from test_plane_host import DLT_BOUND, MOTIONS_BOUND

pytestmark = pytest.mark.gpu

POSE_BOUND = 1e-6  # tests/test_gpu_twoview.py's bound for the device's rotmat_to_aa through aa_to_rotmat
EXACT = ("status", "h_inliers", "iterations", "motion_inliers", "chosen", "n_inliers", "H", "singular", "R", "t", "translation")


def _same(a, b):
    """bit for bit: floats by their bytes (a NaN or a signed zero counts), integers by value"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return b.dtype == a.dtype and a.tobytes() == b.tobytes()
    return np.array_equal(a, b)


@pytest.fixture(scope="module")
def host():
    return cases.build_host()


@pytest.fixture(scope="module")
def mixed(host):
    """the mixed batch with the host build's results: computed once, shared, left unchanged"""
    group = cases.cases()
    b1, b2, off = cases.batch(group)
    want, wmask = cases.host_pairs(host, b1, b2, off)
    return group, b1, b2, off, want, wmask


@pytest.fixture(scope="module")
def device(mixed, gpu_ctx):
    from opensfm_amd import reconstruction

    _, b1, b2, off, _, _ = mixed
    return reconstruction.two_view_plane_pairs(b1, b2, off, cases.THRESHOLD, ctx=gpu_ctx)


def test_mixed_batch_equals_host_build_bit_for_bit(host, mixed, device):
    group, _, _, off, want, wmask = mixed
    got, mask, ms = device
    assert len(got) == len(group) and ms > 0
    seen = set()
    for c, g, w in zip(group, got, want):
        for f in EXACT:
            assert _same(g[f], getattr(w, f)), (c.name, f, g[f], np.asarray(getattr(w, f)))
        if w.status == cases.OK:
            back = np.zeros(9)
            host.host_plane_aa_to_rotmat(np.ascontiguousarray(g["rotation"]).ctypes.data_as(cases.DP), back.ctypes.data_as(cases.DP))
            assert np.abs(back - np.array(w.R)).max() < POSE_BOUND, c.name
        else:
            assert not g["rotation"].any(), c.name
        seen.add(cases.outcome(len(c.b1), w.status, list(w.motion_inliers), bool((c.b2[:, 2] <= 0).all())))
    assert mask.tobytes() == wmask.tobytes()
    assert seen == cases.OUTCOMES, seen  # no branch passes by never being taken


def test_batch_equals_single_pair_calls(mixed, device, gpu_ctx):
    from opensfm_amd import reconstruction

    group, _, _, off, _, _ = mixed
    got, mask, _ = device
    for k, c in enumerate(group):
        one, one_mask, _ = reconstruction.two_view_plane_pairs(c.b1, c.b2, [0, len(c.b1)], cases.THRESHOLD, ctx=gpu_ctx)
        for f in EXACT + ("rotation",):
            assert _same(one[0][f], got[k][f]), (c.name, f)
        assert one_mask.tobytes() == mask[off[k]: off[k + 1]].tobytes(), c.name


def test_leaf_entries_against_the_restatement(gpu_ctx):
    from opensfm_amd import _lib, reconstruction

    lib = _lib.load()
    for name, x1, x2, idx in cases.leaf_dlt_cases():
        a, b = np.ascontiguousarray(x1[idx]), np.ascontiguousarray(x2[idx])
        H, ok = np.zeros(9), C.c_int(-1)
        _lib.check(lib.osfm_homography_solve(gpu_ctx.handle, a.ctypes.data_as(cases.DP), b.ctypes.data_as(cases.DP), len(a), H.ctypes.data_as(cases.DP),
                                             C.byref(ok)), "osfm_homography_solve")
        want = cases.unit_frobenius(cases.dlt(a, b))
        assert ok.value == 1 and np.abs(cases.unit_frobenius(H, want) - want).max() <= DLT_BOUND, name
    for name, H, (R_true, t_true) in cases.leaf_homographies():
        got = reconstruction.motion_from_plane_homography(H, ctx=gpu_ctx)
        assert isinstance(got, list) and len(got) == 8 and all(isinstance(m, tuple) and len(m) == 4 for m in got), name
        assert got[0][0].shape == (3, 3) and got[0][1].shape == (3,) and got[0][2].shape == (3,) and isinstance(got[0][3], float)
        assert np.abs(cases.flat_motions(got) - cases.flat_motions(cases.motions(H))).max() <= MOTIONS_BOUND, name
    assert reconstruction.motion_from_plane_homography(cases.rodrigues([0.1, -0.2, 0.05]), ctx=gpu_ctx) is None


def _pixel_pairs():
    persp = _Cam("perspective", focal=0.9, k1=-0.05, k2=0.01)
    fish = _Cam("fisheye", focal=0.6, k1=-0.02, k2=0.003)
    pairs = []
    for k, (n, cam1, cam2) in enumerate(((120, persp, fish), (3, fish, fish), (65, fish, persp))):
        b1, b2, _, _, _ = cases.plane_scene(np.random.default_rng(700 + k), n)
        pairs.append((_project(cam1, b1), _project(cam2, b2), cam1, cam2))
    return pairs


def test_pixels_twin_equals_bearings_call(gpu_ctx):
    from opensfm_amd import matching, reconstruction

    pairs = _pixel_pairs()
    cams = [pairs[0][2], pairs[0][3]]  # perspective, fisheye: one table
    models, params = zip(*(matching.camera_parameters(c) for c in cams))
    pair_cams = np.array([[cams.index(p[2]), cams.index(p[3])] for p in pairs], np.int32)
    off = np.r_[0, np.cumsum([len(p[0]) for p in pairs])].astype(np.int64)
    got, mask, _ = reconstruction.two_view_plane_pairs_pixels(np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs]), off,
                                                              pair_cams, np.array(models, np.int32), np.array(params), cases.THRESHOLD, ctx=gpu_ctx)
    b1 = np.concatenate([matching.pixel_bearing_many(p[2], p[0], gpu_ctx) for p in pairs])
    b2 = np.concatenate([matching.pixel_bearing_many(p[3], p[1], gpu_ctx) for p in pairs])
    want, wmask, _ = reconstruction.two_view_plane_pairs(b1, b2, off, cases.THRESHOLD, ctx=gpu_ctx)
    for g, w in zip(got, want):
        for f in EXACT + ("rotation",):
            assert _same(g[f], w[f]), f
    assert mask.tobytes() == wmask.tobytes()
    assert [g["status"] for g in got] == [cases.OK, cases.NO_HOMOGRAPHY, cases.OK]
    assert got[0]["h_inliers"] == 84 and got[2]["h_inliers"] == 45  # the planted rows: 70 % of 120 and of 65


def test_refusals_leave_the_outputs_untouched(gpu_ctx):
    from opensfm_amd import _lib

    lib = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    b1, b2, _, _, _ = cases.plane_scene(np.random.default_rng(5), 20)
    b1, b2 = np.ascontiguousarray(b1), np.ascontiguousarray(b2)
    xy = np.ascontiguousarray(b1[:, :2])
    good = _lib.PlaneParams(0.004, 0.99, 1000, 1, 10, 1)
    off = np.array([0, 8, 20], np.int64)
    models, params, pair_cams = np.zeros(1, np.int32), np.zeros((1, 16)), np.zeros((2, 2), np.int32)
    params[0, :3] = (0.0, 0.0, 1.0)

    def attempt(call):
        res = (_lib.PlaneResult * 2)()
        C.memset(res, 0x5A, C.sizeof(res))
        before = bytes(res)
        mask = np.full(20, 0x5A, np.uint8)
        ms = C.c_double(-7.0)
        rc = call(res, mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(ms))
        assert rc != 0
        assert bytes(res) == before and (mask == 0x5A).all() and ms.value == -7.0

    o = off.ctypes.data_as(C.POINTER(C.c_int64))
    h = gpu_ctx.handle
    attempt(lambda res, mask, ms: lib.osfm_two_view_plane_pairs(h, None, b2.ctypes.data_as(dp), o, 2, C.byref(good), res, mask, ms))
    attempt(lambda res, mask, ms: lib.osfm_two_view_plane_pairs(h, b1.ctypes.data_as(dp), b2.ctypes.data_as(dp), None, 2, C.byref(good), res, mask, ms))
    attempt(lambda res, mask, ms: lib.osfm_two_view_plane_pairs(h, b1.ctypes.data_as(dp), b2.ctypes.data_as(dp), o, 2, None, res, mask, ms))
    attempt(lambda res, mask, ms: lib.osfm_two_view_plane_pairs(None, b1.ctypes.data_as(dp), b2.ctypes.data_as(dp), o, 2, C.byref(good), res, mask, ms))
    down = np.array([0, 12, 8], np.int64)
    attempt(lambda res, mask, ms: lib.osfm_two_view_plane_pairs(h, b1.ctypes.data_as(dp), b2.ctypes.data_as(dp), down.ctypes.data_as(C.POINTER(C.c_int64)),
                                                                2, C.byref(good), res, mask, ms))
    for threshold in (0.0, -0.004):
        bad = _lib.PlaneParams(threshold, 0.99, 1000, 1, 10, 1)
        attempt(lambda res, mask, ms: lib.osfm_two_view_plane_pairs(h, b1.ctypes.data_as(dp), b2.ctypes.data_as(dp), o, 2, C.byref(bad), res, mask, ms))
    for cam in (1, -1):
        pc = pair_cams.copy()
        pc[1, 0] = cam
        attempt(lambda res, mask, ms: lib.osfm_two_view_plane_pairs_pixels(h, xy.ctypes.data_as(dp), xy.ctypes.data_as(dp), o, 2, pc.ctypes.data_as(ip),
                                                                           models.ctypes.data_as(ip), params.ctypes.data_as(dp), 1, C.byref(good), res,
                                                                           mask, ms))
    # a null result or mask is refused as well (nothing to look at afterwards)
    mask = np.zeros(20, np.uint8)
    assert lib.osfm_two_view_plane_pairs(h, b1.ctypes.data_as(dp), b2.ctypes.data_as(dp), o, 2, C.byref(good), None,
                                         mask.ctypes.data_as(C.POINTER(C.c_uint8)), None) != 0
    res = (_lib.PlaneResult * 2)()
    assert lib.osfm_two_view_plane_pairs(h, b1.ctypes.data_as(dp), b2.ctypes.data_as(dp), o, 2, C.byref(good), res, None, None) != 0
    # and the same call with everything in place runs, kernel_ms being optional
    assert lib.osfm_two_view_plane_pairs(h, b1.ctypes.data_as(dp), b2.ctypes.data_as(dp), o, 2, C.byref(good), res,
                                         mask.ctypes.data_as(C.POINTER(C.c_uint8)), None) == 0
    assert res[0].status == cases.OK and res[1].status == cases.OK
    assert lib.osfm_two_view_plane_pairs(h, None, None, None, 0, C.byref(good), None, None, None) != 0  # null offsets even for no pairs
    assert lib.osfm_two_view_plane_pairs(h, None, None, o, 0, C.byref(good), None, None, None) == 0


def test_general_pairs_with_the_device_plane_branch(gpu_ctx):
    from opensfm_amd import reconstruction
    import twoview_cases

    # The 5-point solve is not degenerate on a plane: on this scene (outliers kept away from the true epipolar geometry, so that neither
    # branch can claim one) the host builds of both branches find exactly the 140 planted rows, and the reference's rule -- the 5-point
    # result only with strictly more inliers -- gives the pair to the plane branch.  Where the refined 5-point pose picks up one more
    # row than the unrefined plane motion (other seeds do that) the report says "5_point"; that is the reference's rule, not a fault.
    cam = _Cam("perspective", focal=0.9, k1=0.0, k2=0.0)
    b1, b2, planted, (R_true, t_true), _ = cases.plane_scene(np.random.default_rng(33), 200, outliers=0.3, noise=cases.THRESHOLD / 10,
                                                             off_epipolar=True)
    g1, g2, _, _ = twoview_cases.scene(np.random.default_rng(600), 120)  # a general 3-D scene
    pairs = [(_project(cam, b1), _project(cam, b2), cam, cam), (_project(cam, g1), _project(cam, g2), cam, cam)]
    with_plane = reconstruction.two_view_reconstruction_general_pairs(pairs, cases.THRESHOLD, 1000, True, 0.95, plane_based="device", ctx=gpu_ctx)
    without = reconstruction.two_view_reconstruction_general_pairs(pairs, cases.THRESHOLD, 1000, True, 0.95, ctx=gpu_ctx)
    # the planar scene: the plane branch, with the planted rows
    R, t, inliers, report = with_plane[0]
    print("planar pair:", report, "without the plane branch:", without[0][3])
    assert report["method"] == "plane_based" and report["plane_based_inliers"] == len(inliers)
    assert np.array_equal(inliers, planted)
    assert R.shape == (3,) and t.shape == (3,)
    assert np.abs(cases.rodrigues(R) - R_true).max() < 2e-3 and np.abs(t - t_true).max() < 2e-3  # the true motion, t over the plane's distance
    assert without[0][3]["plane_based_inliers"] == 0 and without[0][3].get("method") != "plane_based"
    assert with_plane[0][3]["5_point_inliers"] == without[0][3]["5_point_inliers"]
    # the general scene: the 5-point branch wins, and the result is the one without the argument
    assert with_plane[1][3]["method"] == "5_point" == without[1][3]["method"]
    assert with_plane[1][3]["plane_based_inliers"] < with_plane[1][3]["5_point_inliers"]
    for a, b in zip(with_plane[1][:3], without[1][:3]):
        assert np.array_equal(a, b)
    one = reconstruction.two_view_reconstruction_general(*pairs[0], cases.THRESHOLD, 1000, True, 0.95, plane_based="device", ctx=gpu_ctx)
    assert np.array_equal(one[0], R) and np.array_equal(one[2], inliers) and one[3] == report
    with pytest.raises(ValueError):
        reconstruction.two_view_reconstruction_general_pairs(pairs, cases.THRESHOLD, 1000, plane_based="host", ctx=gpu_ctx)


def test_plane_based_drop_in_returns_the_reference_tuple(mixed, device, gpu_ctx):
    from opensfm_amd import reconstruction

    group, _, _, off, _, _ = mixed
    got, mask, _ = device
    by_name = {c.name: k for k, c in enumerate(group)}
    k = by_name["winner-100"]
    c = group[k]
    R, t, inliers = reconstruction.two_view_reconstruction_plane_based(c.b1, c.b2, cases.THRESHOLD, ctx=gpu_ctx)
    assert isinstance(R, np.ndarray) and R.shape == (3,) and t.shape == (3,) and inliers.dtype.kind == "i"
    assert np.array_equal(R, got[k]["rotation"]) and np.array_equal(t, got[k]["translation"])
    assert np.array_equal(inliers, np.flatnonzero(mask[off[k]: off[k + 1]] >> 1 & 1)) and len(inliers) == got[k]["n_inliers"]
    assert np.abs(cases.rodrigues(R) - c.truth[0]).max() < 2e-3 and np.abs(t - c.truth[1]).max() < 2e-3  # the true motion
    for name in ("rotation-64", "behind-12", "plane-3-noisy"):
        c = group[by_name[name]]
        assert reconstruction.two_view_reconstruction_plane_based(c.b1, c.b2, cases.THRESHOLD, ctx=gpu_ctx) == (None, None, [])
