"""Scenes for the two-view 5-point finish and a step-by-step restatement of it (two_view_reconstruction_and_refinement,
two_view_reconstruction_5pt and the 5-point half of two_view_reconstruction_general) composed from leaves of the CPU oracle:
oracle.ransac_relative_pose, oracle.inliers_bearings and oracle.relative_pose_refinement.  The 3 x 3 transposes and the -R^T t
products are explicit left-to-right scalar sums, so that the host build of twoview_core.h can be held to this bit for bit.

What the restatement does, in this file's words: a configuration starts from the given pose (of the second camera in the first) or from
its inverse; it keeps the correspondences that triangulate within the threshold; with more than five of them it refines the pose over
them (the refinement works on the inverse pose, so the pose is inverted going in and coming out) and keeps the inliers of the refined
pose; it reports the inverse of where it ended.  With two configurations the one with clearly more inliers wins: if the smaller count
over the larger exceeds the reversal ratio nothing is chosen, otherwise the larger wins and a tie goes to the second.

A pair of five or fewer correspondences can never have more than five inliers: like the product, the restatement gives it "no
configuration" without looking at it (RANSAC included)."""
import numpy as np

OK, NO_CONFIGURATION, UNDECIDABLE = 0, 1, 2
THRESHOLD = 0.004
RANSAC_SIZES = (0, 5, 6, 7, 12, 63, 64, 65, 100, 101, 300)
GIVEN_SIZES = (6, 7, 12, 63, 64, 65, 100, 101, 300)


def rodrigues(r):
    th = np.linalg.norm(r)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    return np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th**2 * K @ K


def scene(rng, n, outliers=0.3, noise=1e-3, pose=None):
    """The generator of tests/test_relpose_core_host.py::_scene (X2 = R X + t), also returning (R, t); `pose` fixes them."""
    if pose is None:
        R = rodrigues(rng.normal(0, 0.3, 3))
        t = rng.normal(0, 1, 3)
        t /= np.linalg.norm(t)
    else:
        R, t = np.asarray(pose[0], float), np.asarray(pose[1], float)
    X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)]
    b1 = X + rng.normal(0, noise, X.shape)
    X2 = X @ R.T + t + rng.normal(0, noise, X.shape)
    bad = rng.random(n) < outliers
    X2[bad] = np.c_[rng.uniform(-2, 2, bad.sum()), rng.uniform(-2, 2, bad.sum()), rng.uniform(4, 9, bad.sum())]
    b1 /= np.linalg.norm(b1, axis=1, keepdims=True)
    b2 = X2 / np.linalg.norm(X2, axis=1, keepdims=True)
    return np.ascontiguousarray(b1.reshape(-1, 3)), np.ascontiguousarray(b2.reshape(-1, 3)), np.ascontiguousarray(R), np.ascontiguousarray(t)


# ---- the restatement ----
def transposed3(R):
    return np.array([[R[b][a] for b in range(3)] for a in range(3)], np.float64)


def inverse_translation(R, t):
    """-(R^T t), each entry one left-to-right sum"""
    return np.array([-((R[0][a] * t[0] + R[1][a] * t[1]) + R[2][a] * t[2]) for a in range(3)], np.float64)


def configuration(b1, b2, R, t, threshold, iterations, inverted):
    """-> (R_out, t_out, ascending inlier indices, solver iterations)"""
    import oracle

    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    Rc, tc = (transposed3(R), inverse_translation(R, t)) if inverted else (R.copy(), t.copy())
    inl = np.flatnonzero(oracle.inliers_bearings(b1, b2, Rc, tc, threshold))
    its = 0
    if len(inl) > 5:
        start = np.c_[transposed3(Rc), inverse_translation(Rc, tc)]
        refined, its, _ = oracle.relative_pose_refinement(start, b1[inl], b2[inl], iterations)
        Rc, tc = transposed3(refined[:, :3]), inverse_translation(refined[:, :3], refined[:, 3])
        inl = np.flatnonzero(oracle.inliers_bearings(b1, b2, Rc, tc, threshold))
    return transposed3(Rc), inverse_translation(Rc, tc), inl, its


def decide(n0, n1, check_reversal, reversal_ratio):
    """-> (status, chosen)"""
    counts = [n0] + ([n1] if check_reversal else [])
    valid = [c for c, k in enumerate(counts) if k > 5]
    if len(valid) == 1:
        return OK, valid[0]
    if len(valid) == 2:
        if min(n0, n1) / max(n0, n1) > reversal_ratio:
            return UNDECIDABLE, -1
        return OK, (0 if n0 > n1 else 1)
    return NO_CONFIGURATION, -1


def five_point(b1, b2, R, t, threshold, iterations, check_reversal, reversal_ratio):
    """-> dict(status, chosen, configs = [(R, t, inliers, solver iterations)] per configuration that ran)"""
    if len(b1) <= 5:
        return {"status": NO_CONFIGURATION, "chosen": -1, "configs": []}
    configs = [configuration(b1, b2, R, t, threshold, iterations, inverted) for inverted in ([False, True] if check_reversal else [False])]
    status, chosen = decide(len(configs[0][2]), len(configs[1][2]) if check_reversal else -1, check_reversal, reversal_ratio)
    return {"status": status, "chosen": chosen, "configs": configs}


def general(b1, b2, threshold, iterations, check_reversal, reversal_ratio, ransac_iterations=1000):
    """the 5-point half of two_view_reconstruction_general: the RANSAC's lo_model inverted, then five_point"""
    import oracle

    if len(b1) <= 5:
        return {"status": NO_CONFIGURATION, "chosen": -1, "configs": [], "ransac": None}
    r = oracle.ransac_relative_pose(b1, b2, threshold, ransac_iterations)
    lo = r["lo_model"]
    out = five_point(b1, b2, transposed3(lo[:, :3]), inverse_translation(lo[:, :3], lo[:, 3]), threshold, iterations, check_reversal, reversal_ratio)
    out["ransac"] = r
    return out


# ---- the cases ----
class Case:
    def __init__(self, name, b1, b2, pose, threshold, check_reversal, reversal_ratio, expect=None):
        self.name, self.b1, self.b2, self.pose = name, b1, b2, pose  # pose: (R, t) handed to the finish, or None: RANSAC first
        self.threshold, self.check_reversal, self.reversal_ratio = threshold, check_reversal, reversal_ratio
        self.expect = expect  # (status, chosen) the case is there for, or None

    @property
    def params(self):
        return (self.threshold, self.check_reversal, self.reversal_ratio)


def ransac_cases():
    """one scene per size, the RANSAC first; check_reversal on with the default ratio"""
    out = []
    for k, n in enumerate(RANSAC_SIZES):
        b1, b2, _, _ = scene(np.random.default_rng(100 + k), n, outliers=0.0 if n <= 12 else 0.3)
        out.append(Case("ransac n=%d" % n, b1, b2, None, THRESHOLD, True, 0.95))
    return out


SYMMETRIC_POSE = (np.diag([-1.0, -1.0, 1.0]), np.array([1.0, 0.0, 0.0]))  # its own inverse


def given_pose_cases():
    out = []
    for k, n in enumerate(GIVEN_SIZES):
        b1, b2, R, t = scene(np.random.default_rng(200 + k), n, outliers=0.0 if n <= 12 else 0.3)
        second_in_first = (transposed3(R), inverse_translation(R, t))
        out.append(Case("true pose n=%d" % n, b1, b2, second_in_first, THRESHOLD, True, 0.95, (OK, 0)))
        out.append(Case("true pose, one configuration n=%d" % n, b1, b2, second_in_first, THRESHOLD, False, 1.0, (OK, 0)))
        out.append(Case("inverse pose n=%d" % n, b1, b2, (R, t), THRESHOLD, True, 0.95, (OK, 1)))
    for n in (0, 5):
        b1, b2, R, t = scene(np.random.default_rng(300 + n), n, outliers=0.0)
        out.append(Case("true pose n=%d" % n, b1, b2, (transposed3(R), inverse_translation(R, t)), THRESHOLD, True, 0.95, (NO_CONFIGURATION, -1)))
    b1, b2, R, t = scene(np.random.default_rng(400), 200, pose=SYMMETRIC_POSE)
    out.append(Case("symmetric pose, ratio 0.95", b1, b2, SYMMETRIC_POSE, THRESHOLD, True, 0.95, (UNDECIDABLE, -1)))
    out.append(Case("symmetric pose, ratio 1.0", b1, b2, SYMMETRIC_POSE, THRESHOLD, True, 1.0, (OK, 1)))
    b1, b2, R, t = scene(np.random.default_rng(500), 300)
    out.append(Case("generic scene, loose threshold", b1, b2, (transposed3(R), inverse_translation(R, t)), 0.05, True, 0.95, (OK, 0)))
    return out


def restate(case, refine_iterations=1000):
    if case.pose is None:
        return general(case.b1, case.b2, case.threshold, refine_iterations, case.check_reversal, case.reversal_ratio)
    return five_point(case.b1, case.b2, case.pose[0], case.pose[1], case.threshold, refine_iterations, case.check_reversal, case.reversal_ratio)


def outcome(status, chosen, n0, n1):
    """one of the five outcomes every test run must see: OK-0, OK-1, OK-1-by-tie, undecidable, none"""
    if status == UNDECIDABLE:
        return "undecidable"
    if status == NO_CONFIGURATION:
        return "none"
    if chosen == 1 and n0 == n1 and n0 > 5:
        return "OK-1-by-tie"
    return "OK-%d" % chosen


OUTCOMES = {"OK-0", "OK-1", "OK-1-by-tie", "undecidable", "none"}


def by_params(cases):
    """the cases grouped into calls: one call has one threshold, check_reversal and reversal_ratio"""
    groups = {}
    for c in cases:
        groups.setdefault(c.params, []).append(c)
    return groups


# ---- the host build of twoview_core.h (tests/native/twoview_host.cpp) ----
import ctypes as C  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CSRC = os.path.join(HERE, "..", "opensfm_amd", "csrc")
HOST_DEPS = ([os.path.join(NATIVE, f) for f in ("twoview_host.cpp", "relpose_core_host.cpp", "loop_wave.h")]
             + [os.path.join(CSRC, h) for h in ("twoview_core.h", "relpose_core.h", "relpose_rounds.h", "loransac_walk.h")])


class HostResult(C.Structure):  # twoview_core.h TwoViewOut == osfm_two_view_result
    _fields_ = [("R", C.c_double * 18), ("t", C.c_double * 6), ("rotation", C.c_double * 3), ("translation", C.c_double * 3),
                ("lo_model", C.c_double * 12), ("status", C.c_int32), ("chosen", C.c_int32), ("n_inliers", C.c_int32 * 2),
                ("refine_iterations", C.c_int32 * 2), ("score", C.c_int32), ("iterations", C.c_int32)]


def compile_native(name, src, flags, shared=True):
    out_dir = os.path.join(NATIVE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    target = os.path.join(out_dir, name)
    deps = HOST_DEPS + [src]
    if not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", *(["-fPIC", "-shared"] if shared else []), *flags,
                               "-o", target, src])
    return target


def build_host():
    lib = C.CDLL(compile_native("twoview_host.so", os.path.join(NATIVE, "twoview_host.cpp"), []))
    dp = C.POINTER(C.c_double)
    lib.host_two_view_pairs.restype = C.c_int
    lib.host_two_view_pairs.argtypes = [dp, dp, C.POINTER(C.c_int64), C.c_int, dp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_double, C.c_int, C.POINTER(HostResult), C.POINTER(C.c_uint8)]
    lib.host_two_view_decide.restype = C.c_int
    lib.host_two_view_decide.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int)]
    lib.host_aa_to_rotmat.restype = None
    lib.host_aa_to_rotmat.argtypes = [dp, dp]
    assert lib.host_two_view_result_bytes() == C.sizeof(HostResult)
    return lib


def host_pairs(lib, b1, b2, off, poses, threshold, check_reversal, reversal_ratio, refine_iterations=1000, skip_inlier_tests=False):
    """host_two_view_pairs -> (list of HostResult, mask)"""
    b1, b2 = np.ascontiguousarray(b1, np.float64), np.ascontiguousarray(b2, np.float64)
    off = np.ascontiguousarray(off, np.int64)
    n_pairs = len(off) - 1
    res = (HostResult * max(n_pairs, 1))()
    mask = np.zeros(max(int(off[-1]), 1), np.uint8)
    dp = C.POINTER(C.c_double)
    poses = None if poses is None else np.ascontiguousarray(poses, np.float64)
    rc = lib.host_two_view_pairs(b1.ctypes.data_as(dp), b2.ctypes.data_as(dp), off.ctypes.data_as(C.POINTER(C.c_int64)), n_pairs,
                                 None if poses is None else poses.ctypes.data_as(dp), threshold, 0.99, 1000, 1, 10, refine_iterations,
                                 int(check_reversal), reversal_ratio, int(skip_inlier_tests), res, mask.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == 0
    return [res[p] for p in range(n_pairs)], mask[: int(off[-1])]


def batch(cases):
    """-> b1, b2 (concatenated), offsets, poses (n x 12, or None when the cases have none)"""
    b1 = np.concatenate([c.b1 for c in cases]) if cases else np.zeros((0, 3))
    b2 = np.concatenate([c.b2 for c in cases]) if cases else np.zeros((0, 3))
    off = np.r_[0, np.cumsum([len(c.b1) for c in cases])].astype(np.int64)
    poses = None
    if cases and cases[0].pose is not None:
        poses = np.array([np.r_[np.asarray(c.pose[0], float).reshape(9), np.asarray(c.pose[1], float).reshape(3)] for c in cases])
    return np.ascontiguousarray(b1), np.ascontiguousarray(b2), off, poses
