"""Scenes and plain numpy restatements for the two point-cloud filters of ``opensfm_amd/csrc/cloud.hip`` (``osfm_points_conditioning`` /
``osfm_points_isolation``), written from the text of ``sfm/src/map_helpers.cc``, ``geometry/src/covariance.cc``,
``geometry/src/triangulation.cc:66-73`` and the camera functors (``camera_projections_functions.h``, ``camera_distortions_functions.h``).
Nothing here touches the library, the reference or the oracle: the GPU tests compare the kernels with this module alone.

* ``conditioning_restatement``: FilterBadlyConditionedPoints in the reference's literal order -- the pair-angle test, H = sum J^T J,
  ``np.linalg.det``, ``eigvalsh(inv(H))``, the clamp at 1000, then mean / sigma / threshold accumulated sequentially.  The Jacobians come
  from forward-mode duals over the projection written once (``project``), which ``conditioning_truth_mp`` evaluates with mpmath.
* ``isolation_restatement``: RemoveIsolatedPoints as a float32 brute force, ((dx*dx) + dy*dy) + dz*dz without contraction.
"""
import functools
import math

import numpy as np
import pytest

from opensfm_amd import synthetic
from opensfm_amd.geometry_types import _rodrigues

MODELS = ("perspective", "fisheye", "brown", "fisheye_opencv", "fisheye62", "fisheye624", "dual", "radial", "simple_radial", "spherical")
# model id -> projection (0 perspective, 1 fisheye, 2 dual), distortion kind, distortion / affine parameter counts (camera_instances.h:127-160)
LAYOUT = {0: (0, 1, 2, 1), 1: (1, 1, 2, 1), 2: (0, 3, 5, 4), 3: (1, 2, 4, 4), 4: (1, 4, 8, 4), 5: (1, 5, 12, 4), 6: (2, 1, 2, 1), 7: (0, 1, 2, 4),
          8: (0, 0, 1, 4)}
MAX_COND = 1000.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the projection, written once over an `ops` namespace (sqrt, atan2, pi): numpy duals for the restatement, mpmath for the truth
# ---------------------------------------------------------------------------------------------------------------------------------
def project(model, par, x, y, z, ops):
    """ProjectGeneric<PROJ, DISTO, AFF>::Forward / SphericalProjection::Forward of a camera-frame point"""
    if model == 9:
        lon = ops.atan2(x, z)
        lat = ops.atan2(-y, ops.sqrt(x * x + z * z))
        return lon / (2 * ops.pi), -lat / (2 * ops.pi)
    proj, kind, nd, na = LAYOUT[model]

    def perspective():
        return x / z, y / z

    def fisheye():  # (perspective below r = 1e-8: the scenes keep away from the axis)
        r = ops.sqrt(x * x + y * y)
        theta = ops.atan2(r, z)
        return theta / r * x, theta / r * y

    if proj == 0:
        u, v = perspective()
    elif proj == 1:
        u, v = fisheye()
    else:
        (ua, va), (ub, vb) = perspective(), fisheye()
        t = par[0]
        u, v = t * ua + (1 - t) * ub, t * va + (1 - t) * vb
    k = par[(1 if proj == 2 else 0):]
    ka = k[nd:]
    r2 = u * u + v * v
    if kind == 0:
        rad = 1 + r2 * k[0]
    elif kind == 1:
        rad = 1 + r2 * (k[0] + r2 * k[1])
    elif kind == 2:
        rad = 1 + r2 * (k[0] + r2 * (k[1] + r2 * (k[2] + r2 * k[3])))
    elif kind == 3:
        rad = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))
    else:
        rad = 1 + r2 * (k[0] + r2 * (k[1] + r2 * (k[2] + r2 * (k[3] + r2 * (k[4] + r2 * k[5])))))
    dx, dy = u * rad, v * rad
    if kind >= 3:
        p1, p2 = (k[3], k[4]) if kind == 3 else (k[6], k[7])
        dx = dx + 2 * p1 * u * v + p2 * (r2 + 2 * u * u)
        dy = dy + 2 * p2 * u * v + p1 * (r2 + 2 * v * v)
    if kind == 5:
        dx = dx + k[8] * r2 + k[9] * r2 * r2
        dy = dy + k[10] * r2 + k[11] * r2 * r2
    fx = ka[0]
    fy = ka[0] * ka[1] if na == 4 else ka[0]
    cx, cy = (ka[2], ka[3]) if na == 4 else (0.0, 0.0)
    return fx * dx + cx, fy * dy + cy


class Dual:
    """value (n,) and gradient (n, 3) of a function of the world point, vectorised over observations"""

    def __init__(self, v, g):
        self.v, self.g = v, g

    @staticmethod
    def lift(a, like):
        return a if isinstance(a, Dual) else Dual(np.full_like(like.v, float(a)), np.zeros_like(like.g))

    def __add__(self, o):
        o = Dual.lift(o, self)
        return Dual(self.v + o.v, self.g + o.g)

    __radd__ = __add__

    def __neg__(self):
        return Dual(-self.v, -self.g)

    def __sub__(self, o):
        return self + (-Dual.lift(o, self))

    def __rsub__(self, o):
        return Dual.lift(o, self) + (-self)

    def __mul__(self, o):
        o = Dual.lift(o, self)
        return Dual(self.v * o.v, self.g * o.v[:, None] + o.g * self.v[:, None])

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Dual.lift(o, self)
        return Dual(self.v / o.v, (self.g * o.v[:, None] - o.g * self.v[:, None]) / (o.v * o.v)[:, None])

    def __rtruediv__(self, o):
        return Dual.lift(o, self) / self


class _DualOps:
    pi = math.pi

    @staticmethod
    def sqrt(a):
        v = np.sqrt(a.v)
        return Dual(v, a.g / (2 * v)[:, None])

    @staticmethod
    def atan2(y, x):
        den = x.v * x.v + y.v * y.v
        return Dual(np.arctan2(y.v, x.v), (y.g * x.v[:, None] - x.g * y.v[:, None]) / den[:, None])


def observation_jacobians(scene):
    """(n_obs, 2, 3): derivative of every observation's projection with respect to the world point, in the scene's observation order"""
    P = scene["shot_pose"][scene["obs_shot"]]
    X = scene["points"][scene["obs_point"]]
    R, t = P[:, :9].reshape(-1, 3, 3), P[:, 9:]
    n = len(X)
    J = np.zeros((n, 2, 3))
    cam_of = scene["shot_camera"][scene["obs_shot"]]
    with np.errstate(all="ignore"):
        for c in range(len(scene["cam_model"])):
            sel = np.flatnonzero(cam_of == c)
            if not len(sel):
                continue
            Xc = [Dual((R[sel, a] * X[sel]).sum(1) + t[sel, a], R[sel, a].copy()) for a in range(3)]
            u, v = project(int(scene["cam_model"][c]), [float(p) for p in scene["cam_params"][c]], Xc[0], Xc[1], Xc[2], _DualOps)
            J[sel, 0], J[sel, 1] = u.g, v.g
    return J


def sequential_threshold(values, multiplier):
    """mean + multiplier * population sigma, accumulated in order as std::accumulate does; NaN for no values"""
    values = [float(v) for v in values]
    if not values:
        return float("nan")
    with np.errstate(all="ignore"):
        s = np.float64(0.0)
        for v in values:
            s = s + np.float64(v)
        mean = s / np.float64(len(values))
        ss = np.float64(0.0)
        for v in values:
            ss = ss + (np.float64(v) - mean) * (np.float64(v) - mean)
        return float(mean + np.float64(multiplier) * np.sqrt(ss / np.float64(len(values))))


def landmark_tracks(scene):
    """per landmark the indices of its observations in ascending input order"""
    order = np.argsort(scene["obs_point"], kind="stable")
    bounds = np.searchsorted(scene["obs_point"][order], np.arange(len(scene["points"]) + 1))
    return [order[bounds[p]:bounds[p + 1]] for p in range(len(scene["points"]))]


def conditioning_restatement(scene, min_angle_deg=1.0, min_abs_det=1e-15):
    """FilterBadlyConditionedPoints: cond (NaN where rejected earlier), reason (0 keep, 1 angle, 2 non-finite, 3 determinant, 4 eigenvalues,
    5 above the threshold), threshold, removed -- plus, for the borderline rule of the tests, the widest pair angle and det H per landmark"""
    n = len(scene["points"])
    J = observation_jacobians(scene)
    P = scene["shot_pose"]
    R = P[:, :9].reshape(-1, 3, 3)
    origin = -np.einsum("sji,sj->si", R, P[:, 9:])  # Pose::GetOrigin
    rad_angle = min_angle_deg * math.pi / 180.0
    cond, reason = np.full(n, np.nan), np.zeros(n, np.uint8)
    best_angle, dets = np.full(n, np.nan), np.full(n, np.nan)
    with np.errstate(all="ignore"):
        for p, track in enumerate(landmark_tracks(scene)):
            rays = scene["points"][p] - origin[scene["obs_shot"][track]]
            norm = np.linalg.norm(rays, axis=1)
            rays = np.where(norm[:, None] > 0, rays / norm[:, None], rays)  # Eigen's normalized()
            keep = False
            if len(track) >= 2:
                c = (rays @ rays.T) / np.sqrt(np.outer((rays * rays).sum(1), (rays * rays).sum(1)))
                angle = np.where(np.abs(c) >= 1.0, 0.0, np.arccos(np.clip(c, -1, 1)))
                angle = np.where(np.isnan(c), np.nan, angle)[np.triu_indices(len(track), 1)]
                keep = bool((angle > rad_angle).any())
                if not np.isnan(angle).all():
                    best_angle[p] = np.nanmax(angle)
            if not keep:
                reason[p] = 1
                continue
            H = np.zeros((3, 3))
            for o in track:
                H += J[o].T @ J[o]
            if not np.isfinite(H).all():
                reason[p] = 2
                continue
            det = dets[p] = np.linalg.det(H)
            if not np.isfinite(det) or abs(det) < min_abs_det:
                reason[p] = 3
                continue
            try:
                eigs = np.linalg.eigvalsh(np.linalg.inv(H))
            except np.linalg.LinAlgError:
                reason[p] = 4
                continue
            if not np.isfinite(eigs).all() or eigs.min() <= 0.0:
                reason[p] = 4
                continue
            value = min(math.sqrt(eigs.max() / eigs.min()), MAX_COND)
            if not math.isfinite(value):
                reason[p] = 4
                continue
            cond[p] = value
    threshold = sequential_threshold(cond[reason == 0], 1.0)
    reason[(reason == 0) & (cond > threshold)] = 5
    return {"cond": cond, "reason": reason, "threshold": threshold, "removed": int((reason != 0).sum()), "best_angle": best_angle, "det": dets}


def borderline(res, min_angle_deg=1.0, min_abs_det=1e-15):
    """landmarks whose decision could flip under rounding: cond within 1e-7 relative of the threshold, |det| within 1e-7 relative of
    min_abs_det, or the widest pair angle within 1e-9 rad of the limit"""
    with np.errstate(all="ignore"):
        near_thr = np.isin(res["reason"], (0, 5)) & (np.abs(res["cond"] - res["threshold"]) <= 1e-7 * abs(res["threshold"]))
        near_det = np.isfinite(res["det"]) & (np.abs(np.abs(res["det"]) - min_abs_det) <= 1e-7 * min_abs_det)
        near_angle = np.abs(res["best_angle"] - min_angle_deg * math.pi / 180.0) <= 1e-9
    return np.flatnonzero(near_thr | near_det | near_angle)


def conditioning_truth_mp(scene, landmarks, digits=50):
    """cond of the given landmarks from the same formulas at `digits` digits: Jacobians by mpmath differentiation of `project`, the
    eigenvalues of H by mpmath's symmetric solver"""
    import mpmath as mp

    class Ops:
        sqrt, atan2 = staticmethod(mp.sqrt), staticmethod(mp.atan2)

    out = []
    tracks = landmark_tracks(scene)
    with mp.workdps(digits):
        Ops.pi = mp.pi
        for p in landmarks:
            H = mp.zeros(3, 3)
            X0 = [mp.mpf(float(v)) for v in scene["points"][p]]
            for o in tracks[p]:
                s = int(scene["obs_shot"][o])
                c = int(scene["shot_camera"][s])
                Rt = [mp.mpf(float(v)) for v in scene["shot_pose"][s]]
                par = [mp.mpf(float(v)) for v in scene["cam_params"][c]]
                model = int(scene["cam_model"][c])

                def f(comp, x, y, z):
                    Xc = [Rt[3 * a] * x + Rt[3 * a + 1] * y + Rt[3 * a + 2] * z + Rt[9 + a] for a in range(3)]
                    return project(model, par, Xc[0], Xc[1], Xc[2], Ops)[comp]

                Jm = mp.matrix(2, 3)
                for comp in range(2):
                    for a in range(3):
                        order = tuple(1 if b == a else 0 for b in range(3))
                        Jm[comp, a] = mp.diff(lambda x, y, z: f(comp, x, y, z), tuple(X0), order)
                H += Jm.T * Jm
            E = mp.eigsy(H, eigvals_only=True)
            lo, hi = min(E), max(E)
            out.append(float(min(mp.sqrt(hi / lo), mp.mpf(MAX_COND))))
    return np.array(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# conditioning scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def _pose_row(rotation, centre):
    R = _rodrigues(rotation)
    return np.r_[R.reshape(9), -R @ np.asarray(centre, float)]


def _table(models):
    cam_params = np.zeros((len(models), 16))
    for c, m in enumerate(models):
        cam_params[c, :len(synthetic.BUNDLE_TEST_CAMERAS[m])] = synthetic.BUNDLE_TEST_CAMERAS[m]
    return np.array([MODELS.index(m) for m in models], np.int32), cam_params


N_STREET = 220  # street shots; three more stand far behind them


@functools.lru_cache(maxsize=None)
def conditioning_scene(n_landmarks, seed=5):
    """A street of 220 shots (two camera models alternating) and the first `n_landmarks` landmarks of one fixed list that starts with the
    special cases -- 0: no observation; 1: one observation; 2: two observations, wide; 3: rays parallel to rounding (a point 1e12 away);
    4: a point exactly at a camera centre, seen from two more shots; 5: two rays 1.01 degrees apart from cameras 30 x apart in distance
    (cond ~1 700: the clamp); 6: seen only by the far group, determinant ~1e-19 -- and goes on with ragged tracks of 2 .. 200 observations
    (lengths 2, 7, 8, 9, 16, 17, 64, 65, 200 among the first).  The observations are shuffled: `any order`."""
    rng = np.random.default_rng(seed)
    models = ("perspective", "brown")
    cam_model, cam_params = _table(models)
    centres = np.c_[np.arange(N_STREET) * 0.05, rng.normal(0, 0.02, N_STREET), rng.normal(0, 0.02, N_STREET)]
    rotations = rng.normal(0, 0.02, (N_STREET, 3))
    rotations[0] = 0.0  # shot 0: R = I exactly, so that a point at its centre is at the camera-frame origin exactly
    centres[0] = [0.0, 0.25, -0.5]
    far = [[-100.0, 0.0, -1000.0], [100.0, 0.0, -1000.0], [0.0, 100.0, -1000.0]]
    shot_pose = np.array([_pose_row(rotations[s], centres[s]) for s in range(N_STREET)] + [_pose_row(np.zeros(3), c) for c in far])
    shot_camera = (np.arange(len(shot_pose)) % 2).astype(np.int32)
    points, tracks = [], []
    lengths = [2, 7, 8, 9, 16, 17, 64, 65, 200]
    for p in range(n_landmarks):
        if p == 0:
            X, track = [1.0, 0.0, 8.0], []
        elif p == 1:
            X, track = [1.0, 0.0, 8.0], [10]
        elif p == 2:
            X, track = [2.0, 0.3, 6.0], [20, 60]
        elif p == 3:
            X, track = [3.0, 0.0, 1e12], [5, 100, 200]
        elif p == 4:
            X, track = centres[0].copy(), [0, 40, 120]
        elif p == 5:
            # two cameras on almost one line through the point: the near one 5 away, the far one 150 away, 1.01 degrees between the rays
            a = 1.01 * math.pi / 180.0
            X = centres[30] + np.array([0.0, 0.0, 5.0])
            extra = X - 150.0 * np.array([math.sin(a), 0.0, math.cos(a)])
            shot_pose = np.vstack([shot_pose, _pose_row(np.zeros(3), extra)])
            shot_camera = np.r_[shot_camera, 0].astype(np.int32)
            track = [30, len(shot_pose) - 1]
        elif p == 6:
            X, track = [0.0, 0.0, 0.0], [N_STREET, N_STREET + 1, N_STREET + 2]
        else:
            L = lengths[p - 7] if p - 7 < len(lengths) else int(round(math.exp(rng.uniform(math.log(2), math.log(200)))))
            first = int(rng.integers(0, N_STREET - L + 1))
            X = [centres[first + L // 2, 0] + rng.uniform(-0.3, 0.3), rng.uniform(-1.0, 1.0), rng.uniform(4.0, 12.0)]
            track = list(range(first, first + L))
        points.append(np.asarray(X, float))
        tracks.append(track)
    obs_point = np.concatenate([np.full(len(t), p, np.int32) for p, t in enumerate(tracks)] + [np.zeros(0, np.int32)])
    obs_shot = np.concatenate([np.asarray(t, np.int32) for t in tracks] + [np.zeros(0, np.int32)])
    order = rng.permutation(len(obs_point))
    return {"points": np.array(points).reshape(-1, 3), "shot_pose": shot_pose, "shot_camera": shot_camera, "cam_model": cam_model,
            "cam_params": cam_params, "obs_shot": obs_shot[order].astype(np.int32), "obs_point": obs_point[order].astype(np.int32)}


@functools.lru_cache(maxsize=None)
def model_scene(model, n_landmarks=48, n_shots=30, seed=11):
    """every shot uses `model`; tracks of 2 .. 12 shots around a street, well-conditioned geometry"""
    rng = np.random.default_rng(seed + MODELS.index(model))
    cam_model, cam_params = _table((model,))
    centres = np.c_[np.arange(n_shots) * 0.3, rng.normal(0, 0.05, n_shots), rng.normal(0, 0.05, n_shots)]
    shot_pose = np.array([_pose_row(rng.normal(0, 0.03, 3), centres[s]) for s in range(n_shots)])
    points, obs_shot, obs_point = [], [], []
    for p in range(n_landmarks):
        L = int(rng.integers(2, 13))
        first = int(rng.integers(0, n_shots - L + 1))
        points.append([centres[first + L // 2, 0] + rng.uniform(-0.5, 0.5), rng.uniform(0.2, 1.2) * (1 if p % 2 else -1), rng.uniform(4.0, 9.0)])
        obs_shot += list(range(first, first + L))
        obs_point += [p] * L
    order = rng.permutation(len(obs_point))
    return {"points": np.array(points), "shot_pose": shot_pose, "shot_camera": np.zeros(n_shots, np.int32), "cam_model": cam_model,
            "cam_params": cam_params, "obs_shot": np.asarray(obs_shot, np.int32)[order], "obs_point": np.asarray(obs_point, np.int32)[order]}


@functools.lru_cache(maxsize=None)
def conditioning_reference(kind, arg):
    """the restatement of a scene, computed once per session: kind "scene" (arg = landmarks) or "model" (arg = model name)"""
    scene = conditioning_scene(arg) if kind == "scene" else model_scene(arg)
    return conditioning_restatement(scene)


# ---------------------------------------------------------------------------------------------------------------------------------
# isolation
# ---------------------------------------------------------------------------------------------------------------------------------
def isolation_restatement(points, k=7):
    """RemoveIsolatedPoints: avg (mean of the k smallest non-self squared distances, float32 arithmetic, float64 sum in ascending order),
    removed, threshold, count.  n <= k: nothing computed (NaN), nothing removed."""
    P = np.asarray(points, np.float64).reshape(-1, 3).astype(np.float32)
    n = len(P)
    if n <= k:
        return {"avg": np.full(n, np.nan), "removed": np.zeros(n, bool), "threshold": float("nan"), "count": 0}
    avg = np.zeros(n)
    for a in range(0, n, 512):
        d = P[a:a + 512, None, :] - P[None, :, :]
        d2 = d[..., 0] * d[..., 0]
        d2 = d2 + d[..., 1] * d[..., 1]
        d2 = d2 + d[..., 2] * d[..., 2]
        assert d2.dtype == np.float32
        small = np.sort(np.partition(d2, k, axis=1)[:, :k + 1], axis=1)
        s = np.zeros(len(small))
        for j in range(1, k + 1):  # neighbors[0] is the query itself
            s = s + small[:, j].astype(np.float64)
        avg[a:a + 512] = s / k
    threshold = sequential_threshold(avg, 1.25)
    removed = avg > threshold
    return {"avg": avg, "removed": removed, "threshold": threshold, "count": int(removed.sum())}


def _cloud(name):
    rng = np.random.default_rng(abs(hash_name(name)))
    if name in ("n7", "n8", "n9"):
        return rng.uniform(-1, 1, (int(name[1:]), 3))
    if name == "uniform":
        return rng.uniform(-5, 5, (3000, 3))
    if name == "gaussian_far":  # the far points stay open after the ring budget: the brute-force pass
        return np.r_[rng.normal(0, 1, (2000, 3)), rng.uniform(-60, 60, (40, 3))]
    if name == "lattice":  # 12^3, full of ties
        g = np.arange(12, dtype=float)
        return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * 0.5
    if name == "tripled":
        return np.repeat(rng.uniform(-2, 2, (300, 3)), 3, axis=0)[rng.permutation(900)]
    if name == "overfull":  # one overfull cell
        return np.r_[np.tile([[0.25, -1.5, 3.0]], (4000, 1)), rng.uniform(-3, 3, (100, 3))][rng.permutation(4100)]
    if name == "plane":
        return np.c_[rng.uniform(-4, 4, (1500, 2)), np.full(1500, 2.5)]
    if name == "line":
        return np.c_[rng.uniform(-4, 4, 500), np.full(500, -1.0), np.full(500, 0.75)]
    if name == "two_clusters":  # the cap of 1 024 cells per axis
        return np.r_[rng.normal(0, 1, (500, 3)), rng.normal(0, 1, (500, 3)) + [1e6, 0, 0]]
    raise KeyError(name)


def hash_name(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


CLOUDS = ("n7", "n8", "n9", "uniform", "lattice", "tripled", "overfull", "plane", "line", "gaussian_far", "two_clusters")
KDTREE_CLOUDS = ("uniform", "gaussian_far", "lattice", "tripled", "plane", "n9", "n8")  # the seven the definition was checked on


@functools.lru_cache(maxsize=None)
def cloud(name):
    pts = _cloud(name)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def isolation_reference(name, k=7):
    return isolation_restatement(cloud(name), k)


# ---------------------------------------------------------------------------------------------------------------------------------
# a reconstruction with rigs and two camera models, for the calls through Python
# ---------------------------------------------------------------------------------------------------------------------------------
def bundle_reconstruction(models=("perspective", "brown"), seed=3):
    """geometry_types objects of a ``synthetic.make_bundle_scene`` problem, ground-truth poses and points plus a few landmarks pushed far
    away (isolated) and a few seen under a narrow angle"""
    from opensfm_amd.geometry_types import Camera, Observation, Pose, Reconstruction, RigCamera, RigInstance, set_camera_parameter_values

    prob = synthetic.make_bundle_scene(models=models, seed=seed, n_gcp=0, up_vectors=False, free_bias=False)
    rng = np.random.default_rng(seed)
    r = Reconstruction()
    for c, m in enumerate(models):
        cam = Camera(m)
        set_camera_parameter_values(cam, prob["cam_params"][c])
        cam.id = "c%d" % c
        r.add_camera(cam)
    for k, v in enumerate(prob["rig_camera_pose"]):
        r.add_rig_camera(RigCamera("rc%d" % k, Pose.from_cam_to_world(v[:3], v[3:])))
    for k, v in enumerate(prob["rig_instance_pose"]):
        r.add_rig_instance(RigInstance("i%d" % k, Pose.from_cam_to_world(v[:3], v[3:])))
    for s in range(len(prob["shot_camera"])):
        r.create_shot("s%03d" % s, "c%d" % prob["shot_camera"][s], None, "rc%d" % prob["shot_rig_camera"][s], "i%d" % prob["shot_rig_instance"][s])
    points = np.array(prob["points"], float)
    far = rng.choice(len(points), 5, replace=False)
    points[far] += rng.normal(0, 1, (5, 3)) * 40.0
    for p, X in enumerate(points):
        r.create_point("p%d" % p, X)
    for s, p, xy, sd in zip(prob["obs_shot"], prob["obs_point"], prob["obs_xy"], prob["obs_sigma"]):
        r.add_observation("s%03d" % s, "p%d" % p, Observation(xy[0], xy[1], sd))
    return r


def scene_of_reconstruction(r):
    """the arrays of a geometry_types.Reconstruction for the restatements, built from the objects directly: landmarks in map order, shots
    in map order with ``shot.pose`` (rig camera o rig instance), observations shot by shot"""
    lm_ids = list(r.points)
    index = {lm: i for i, lm in enumerate(lm_ids)}
    cam_ids = list(r.cameras)
    cam_model = np.array([MODELS.index(r.cameras[c].projection_type) for c in cam_ids], np.int32)
    cam_params = np.zeros((len(cam_ids), 16))
    for c, cid in enumerate(cam_ids):
        v = r.cameras[cid].get_parameters_values()
        cam_params[c, :len(v)] = v
    shot_pose, shot_camera, obs_shot, obs_point = [], [], [], []
    for s, shot in enumerate(r.shots.values()):
        pose = shot.pose
        shot_pose.append(np.r_[pose.get_R_world_to_cam().reshape(9), pose.get_t_world_to_cam()])
        shot_camera.append(cam_ids.index(shot.camera.id))
        for lm in shot.observations:
            if lm in index:
                obs_shot.append(s)
                obs_point.append(index[lm])
    return lm_ids, {"points": np.array([r.points[lm].coordinates for lm in lm_ids]).reshape(-1, 3), "shot_pose": np.array(shot_pose),
                    "shot_camera": np.array(shot_camera, np.int32), "cam_model": cam_model, "cam_params": cam_params,
                    "obs_shot": np.array(obs_shot, np.int32), "obs_point": np.array(obs_point, np.int32)}


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparisons the emulated (tests/test_cloud_host.py) and the GPU (tests/test_gpu_cloud.py) runs share
# ---------------------------------------------------------------------------------------------------------------------------------
def check_isolation(got, ref):
    """bit-equal averages, flags, threshold and count"""
    assert np.array_equal(got["avg"], ref["avg"], equal_nan=True)
    assert np.array_equal(got["removed"], ref["removed"])
    assert got["threshold"] == ref["threshold"] or (np.isnan(got["threshold"]) and np.isnan(ref["threshold"]))
    assert got["count"] == ref["count"]


def check_conditioning(got, ref):
    """cond and the threshold within rtol 1e-8, identical reasons (the callers' scenes have no borderline landmark)"""
    print("max relative cond difference %.3g, thresholds %r %r" % (np.nanmax(np.abs(got["cond"] / ref["cond"] - 1), initial=0.0),
                                                                   got["threshold"], ref["threshold"]))
    assert np.array_equal(np.isnan(got["cond"]), np.isnan(ref["cond"]))
    ok = ~np.isnan(ref["cond"])
    np.testing.assert_allclose(got["cond"][ok], ref["cond"][ok], rtol=1e-8, atol=0)
    if np.isnan(ref["threshold"]):
        assert np.isnan(got["threshold"])
    else:
        np.testing.assert_allclose(got["threshold"], ref["threshold"], rtol=1e-8, atol=0)
    assert np.array_equal(got["reason"], ref["reason"])  # the removal set, reason by reason
    assert got["removed"] == ref["removed"]


def check_python_filters():
    """compat.pysfm.filter_badly_conditioned_points / remove_isolated_points and reconstruction.cull_final_point_cloud on a
    make_bundle_scene reconstruction with rigs and two camera models, through whatever library ``_lib.load()`` gives: the map keeps
    exactly the landmarks the restatement keeps, and no shot keeps an observation of a removed one"""
    from opensfm_amd import reconstruction as gpu_reconstruction
    from opensfm_amd.compat import pysfm

    r = bundle_reconstruction()
    lm_ids, scene = scene_of_reconstruction(r)
    ref = conditioning_restatement(scene, 1.0)
    assert len(borderline(ref)) == 0 and 0 < ref["removed"] < len(lm_ids)
    keep1 = [lm for lm, why in zip(lm_ids, ref["reason"]) if why == 0]
    assert pysfm.filter_badly_conditioned_points(r.map, 1.0) == ref["removed"]
    assert list(r.points) == keep1
    iso = isolation_restatement(np.array([r.points[lm].coordinates for lm in keep1]), 7)
    assert 0 < iso["count"] < len(keep1)
    keep2 = [lm for lm, gone in zip(keep1, iso["removed"]) if not gone]
    assert pysfm.remove_isolated_points(r.map) == iso["count"]
    assert list(r.points) == keep2
    for shot in r.shots.values():
        assert set(shot.observations) <= set(keep2)
    # cull_final_point_cloud: the outlier step always, the two filters only under filter_final_point_cloud
    r2 = bundle_reconstruction()
    n0 = len(r2.points)
    config = {"bundle_outlier_filtering_type": "FIXED", "bundle_outlier_fixed_threshold": 0.006, "triangulation_min_ray_angle": 1.0,
              "filter_final_point_cloud": False}
    rep = gpu_reconstruction.cull_final_point_cloud(r2, config)
    assert len(r2.points) == n0 and rep["badly_conditioned"] == 0 and rep["isolated"] == 0
    rep = gpu_reconstruction.cull_final_point_cloud(r2, dict(config, filter_final_point_cloud=True))
    assert rep["badly_conditioned"] == ref["removed"] and rep["isolated"] == iso["count"] and list(r2.points) == keep2
    with pytest.raises(KeyError):  # the keys are read as the reference reads them
        gpu_reconstruction.cull_final_point_cloud(bundle_reconstruction(), {"bundle_outlier_filtering_type": "FIXED"})
