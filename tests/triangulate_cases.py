"""Scenes and two numpy restatements for the track triangulation of ``opensfm_amd/csrc/triangulate.hip`` (``osfm_triangulate_bearings`` /
``osfm_triangulate_tracks``), written from the text of ``opensfm/reconstruction.py:1032-1073``, ``geometry/src/triangulation.cc``,
``geometry/triangulation.h:58-82`` and ``geometry/transformations_functions.h:265-305``.

* ``restate_track`` follows the algorithm step by step in float64: the pair-angle test through arccos, the midpoint from BBt, BBtA and A,
  the two per-observation tests in order, then TinySolver as ``triangulate_core.h`` describes it (the same step sequence; numpy sums in
  numpy's order).  It records every comparison it makes, so that ``borderline`` can say whether a decision hung on rounding.
* ``minimiser_mp`` is independent of all that: the stationary point of sum |normalize(X - o_i) - w_i|^2 by Newton at 50 digits.

The bearings of the pixel scenes come from the oracle's ``pixel_bearings_generic`` (C, written from the reference's camera functors), not
from the library under test."""
import functools
import math

import numpy as np

import cloud_cases
from cloud_cases import MODELS, _pose_row, _table

DEFAULT = {"threshold": 0.006, "min_angle_deg": 1.0, "min_depth": 0.001, "iterations": 10}
REFERENCE = {"threshold": 0.01, "min_angle_deg": 2.0, "min_depth": 0.001, "iterations": 10}  # the values of the reference's test_triangulation.py
BORDERLINE = 1e-9
EPS = 2.220446049250313e-16


# ---------------------------------------------------------------------------------------------------------------------------------
# the step-by-step restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def dot3(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def angle_between(u, v):
    """geometry::AngleBetweenVectors, broadcasting; 0 where |c| >= 1, NaN where c is NaN"""
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.asarray((u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]) /
                       np.sqrt((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1] + u[..., 2] * u[..., 2]) *
                               (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])))
        return np.where(np.abs(c) >= 1.0, 0.0, np.arccos(np.where(np.abs(c) >= 1.0, 0.0, c)))


def inverse3(m):
    m = m.reshape(9)
    c00, c10, c20 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
    with np.errstate(divide="ignore", invalid="ignore"):
        invdet = np.float64(1.0) / (c00 * m[0] + c10 * m[1] + c20 * m[2])
        return np.array([c00 * invdet, (m[2] * m[7] - m[1] * m[8]) * invdet, (m[1] * m[5] - m[2] * m[4]) * invdet,
                         c10 * invdet, (m[0] * m[8] - m[2] * m[6]) * invdet, (m[2] * m[3] - m[0] * m[5]) * invdet,
                         c20 * invdet, (m[1] * m[6] - m[0] * m[7]) * invdet, (m[0] * m[4] - m[1] * m[3]) * invdet])


def midpoint(o, w):
    """TriangulateBearingsMidpointSolve (triangulation.h:58-82)"""
    n = len(o)
    B = np.array([[(w[:, a] * w[:, b]).sum() for b in range(3)] for a in range(3)])
    BA = np.array([(((w[:, a] * w[:, 0]) * o[:, 0] + (w[:, a] * w[:, 1]) * o[:, 1]) + (w[:, a] * w[:, 2]) * o[:, 2]).sum() for a in range(3)])
    A = o.sum(axis=0)
    Cinv = inverse3(float(n) * np.eye(3) - B).reshape(3, 3)
    X = np.zeros(3)
    with np.errstate(invalid="ignore"):
        for r in range(3):
            acc = sub = np.float64(0.0)
            for c in range(3):
                bc = (B[r, 0] * Cinv[0, c] + B[r, 1] * Cinv[1, c]) + B[r, 2] * Cinv[2, c]
                acc = acc + ((1.0 if r == c else 0.0) + bc) * A[c]
                sub = sub + Cinv[r, c] * BA[c]
            X[r] = acc / float(n) - sub
    return X


def ldlt3_solve(a, b):
    d0 = a[0]
    l10, l20 = a[1] / d0, a[2] / d0
    d1 = a[3] - l10 * l10 * d0
    l21 = (a[4] - l20 * l10 * d0) / d1
    d2 = a[5] - l20 * l20 * d0 - l21 * l21 * d1
    y0 = b[0]
    y1 = b[1] - l10 * y0
    y2 = b[2] - l20 * y0 - l21 * y1
    x2 = y2 / d2
    x1 = y1 / d1 - l21 * x2
    x0 = y0 / d0 - l10 * x1 - l20 * x2
    return np.array([x0, x1, x2])


def _evaluate(o, w, X, with_jacobian):
    """J^T J (00 01 02 11 12 22), J^T e, |e|^2 with e = -(normalize(X - o) - w), unscaled"""
    p = X[None, :] - o
    inv_norm = 1.0 / np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    e = -(p * inv_norm[:, None] - w)
    ee = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).sum() if len(o) else np.float64(0.0)
    if not with_jacobian:
        return None, None, ee
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    x2, y2, z2 = x * x, y * y, z * z
    norm2 = x2 + y2 + z2
    s = 1.0 / (np.sqrt(norm2) * norm2)
    J = np.stack([(y2 + z2) * s, (-x * y) * s, (-x * z) * s, (-y * x) * s, (x2 + z2) * s, (-y * z) * s, (-z * x) * s, (-z * y) * s, (x2 + y2) * s], axis=1)
    H = np.array([((J[:, a] * J[:, b] + J[:, 3 + a] * J[:, 3 + b]) + J[:, 6 + a] * J[:, 6 + b]).sum() for a in range(3) for b in range(a, 3)])
    q = np.array([((J[:, a] * e[:, 0] + J[:, 3 + a] * e[:, 1]) + J[:, 6 + a] * e[:, 2]).sum() for a in range(3)])
    return H, q, ee


def refine(o, w, X, max_num_iterations, notes=None):
    """PointRefinement: TinySolver as restated in triangulate_core.h -> (X, summary.iterations).  `notes` collects (what, value, bound)
    of every comparison."""
    notes = [] if notes is None else notes
    X = np.array(X, np.float64)
    diag = (0, 3, 5)
    pair = [(a, b) for a in range(3) for b in range(a, 3)]
    with np.errstate(all="ignore"):
        H, q, ee = _evaluate(o, w, X, True)
        scaling = 1.0 / (1.0 + np.sqrt(H[list(diag)]))

        def update(H, q, ee):
            jtj = np.array([H[k] * scaling[a] * scaling[b] for k, (a, b) in enumerate(pair)])
            g = q * scaling
            return jtj, g, max(abs(g[0]), max(abs(g[1]), abs(g[2]))), ee / 2.0

        jtj, g, gmax, cost = update(H, q, ee)
        notes += [("gradient", gmax, 1e-10), ("cost", cost, EPS)]
        if gmax < 1e-10 or cost < EPS:
            return X, 0
        u, v = 1.0 / 1e4, 2.0
        it = 1
        while it < max_num_iterations:
            reg = jtj.copy()
            for a in range(3):
                lm = math.sqrt(u * min(max(jtj[diag[a]], 1e-6), 1e32))
                reg[diag[a]] += lm * lm
            step = ldlt3_solve(reg, g)
            dx = scaling * step
            xnorm = math.sqrt((X[0] * X[0] + X[1] * X[1]) + X[2] * X[2])
            dxnorm = math.sqrt((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2])
            notes.append(("step", dxnorm, 1e-8 * (xnorm + 1e-8)))
            if dxnorm < 1e-8 * (xnorm + 1e-8):
                break
            xn = X + dx
            _, _, ee_new = _evaluate(o, w, xn, False)
            cost_change = 2.0 * cost - ee_new
            js = np.array([(jtj[0] * step[0] + jtj[1] * step[1]) + jtj[2] * step[2], (jtj[1] * step[0] + jtj[3] * step[1]) + jtj[4] * step[2],
                           (jtj[2] * step[0] + jtj[4] * step[1]) + jtj[5] * step[2]])
            model_cost_change = (step[0] * (2.0 * g[0] - js[0]) + step[1] * (2.0 * g[1] - js[1])) + step[2] * (2.0 * g[2] - js[2])
            rho = cost_change / model_cost_change
            notes.append(("rho", abs(cost_change) / (2.0 * cost), 0.0))  # the sign of rho hangs on rounding when the change is ~eps * cost
            if rho > 0.0:
                X = xn
                notes.append(("cost change", abs(cost_change), 1e-6))
                if abs(cost_change) < 1e-6:
                    break
                H, q, ee = _evaluate(o, w, X, True)
                jtj, g, gmax, cost = update(H, q, ee)
                notes += [("gradient", gmax, 1e-10), ("cost", cost, EPS)]
                if gmax < 1e-10 or cost < EPS:
                    break
                tmp = 2.0 * rho - 1.0
                u = u * max(1.0 / 3.0, 1.0 - tmp * tmp * tmp)
                v = 2.0
            else:
                u *= v
                v *= 2.0
            it += 1
    return X, it


def restate_track(o, w, prm=DEFAULT):
    """-> (status, X or NaNs, iterations, notes)"""
    o = np.asarray(o, np.float64).reshape(-1, 3)
    w = np.asarray(w, np.float64).reshape(-1, 3)
    nan3 = np.full(3, np.nan)
    notes = []
    n = len(o)
    if n < 2:
        return 1, nan3, 0, notes
    min_angle = prm["min_angle_deg"] * math.pi / 180.0
    i, j = np.tril_indices(n, -1)
    angles = angle_between(w[i], w[j])
    notes += [("ray angle", a, b) for b in (min_angle, math.pi - min_angle) for a in angles[np.abs(angles - b) <= 10 * BORDERLINE * max(b, 1e-300)]]
    with np.errstate(invalid="ignore"):
        if not ((angles >= min_angle) & (angles <= math.pi - min_angle)).any():
            return 2, nan3, 0, notes
    X = midpoint(o, w)
    p = X[None, :] - o
    reproj = angle_between(p, w)
    with np.errstate(invalid="ignore"):
        depth = dot3(p, w)
        for k in range(n):
            notes += [("reprojection", reproj[k], prm["threshold"])]
            if reproj[k] > prm["threshold"]:
                return 3, nan3, 0, notes
            notes += [("depth", depth[k], prm["min_depth"])]
            if depth[k] < prm["min_depth"]:
                return 4, nan3, 0, notes
    if not np.isfinite(X).all():
        return 5, nan3, 0, notes
    X, it = refine(o, w, X, prm["iterations"], notes)
    if not np.isfinite(X).all():
        return 5, nan3, it, notes
    return 0, X, it, notes


def borderline_notes(notes):
    """the comparisons that lie within 1e-9 relative of their bound (for "rho": a cost change within 1e-9 of the cost itself)"""
    out = []
    for what, value, bound in notes:
        if what == "rho":
            if value <= BORDERLINE:
                out.append((what, value, bound))
        elif np.isfinite(value) and abs(value - bound) <= BORDERLINE * abs(bound):
            out.append((what, value, bound))
    return out


def minimiser_mp(o, w, x0, digits=50):
    """the stationary point of sum |normalize(X - o_i) - w_i|^2 nearest x0, by Newton at `digits` digits -> float64 (3,)"""
    import mpmath as mp

    with mp.workdps(digits):
        O = [[mp.mpf(float(v)) for v in row] for row in o]
        W = [[mp.mpf(float(v)) for v in row] for row in w]

        def gradient(x, y, z):  # |t| = 1: f = sum (1 + |w|^2 - 2 t.w), so grad = -2 sum (w - t (t.w)) / |p|
            g = [mp.mpf(0)] * 3
            for oi, wi in zip(O, W):
                p = [x - oi[0], y - oi[1], z - oi[2]]
                norm = mp.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
                t = [c / norm for c in p]
                tw = t[0] * wi[0] + t[1] * wi[1] + t[2] * wi[2]
                g = [g[k] - 2 * (wi[k] - t[k] * tw) / norm for k in range(3)]
            return g

        root = mp.findroot(gradient, [mp.mpf(float(v)) for v in x0], tol=mp.mpf(10) ** (-(digits - 10)), maxsteps=60)
        return np.array([float(v) for v in root])


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes: {"params", "offsets", and the pixel form (shot_pose, shot_camera, cam_model, cam_params, obs_shot, obs_xy) and / or the ray
# form (centers, bearings); "truth" where the rays are exact}
# ---------------------------------------------------------------------------------------------------------------------------------
class _FloatOps:
    pi = math.pi
    sqrt = staticmethod(np.sqrt)
    atan2 = staticmethod(np.arctan2)


def _project(model, par, pose_row, X):
    R, t = pose_row[:9].reshape(3, 3), pose_row[9:]
    xc = R @ np.asarray(X, float) + t
    u, v = cloud_cases.project(model, list(par), xc[0], xc[1], xc[2], _FloatOps)
    return float(u), float(v)


def world_rays(scene):
    """centers and bearings of a pixel scene's rows, the way the kernel forms them: b = Camera::Bearing (the oracle's), w = R^T b,
    o = -R^T t, term by term in the kernel's order"""
    import oracle

    oracle.build()
    shot, xy = scene["obs_shot"], scene["obs_xy"]
    b = np.zeros((len(shot), 3))
    cam_of = scene["shot_camera"][shot] if len(shot) else np.zeros(0, np.int32)
    for c in range(len(scene["cam_model"])):
        rows = np.flatnonzero(cam_of == c)
        if len(rows):
            b[rows] = oracle.pixel_bearings_generic(int(scene["cam_model"][c]), scene["cam_params"][c], xy[rows])
    P = scene["shot_pose"][shot].reshape(-1, 12)
    w = np.stack([(P[:, k] * b[:, 0] + P[:, 3 + k] * b[:, 1]) + P[:, 6 + k] * b[:, 2] for k in range(3)], axis=1)
    o = np.stack([-((P[:, k] * P[:, 9] + P[:, 3 + k] * P[:, 10]) + P[:, 6 + k] * P[:, 11]) for k in range(3)], axis=1)
    return o, w


N_STREET = 330
LENGTHS = (0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 300)  # the lane-group and wavefront boundaries (and the 16 / 17 of the kernel split below)


@functools.lru_cache(maxsize=None)
def ragged_scene(n_tracks, seed=7):
    """A street of 330 shots (perspective and brown alternating) and the first `n_tracks` tracks of one fixed list: the lengths of LENGTHS,
    then 15, 16, 17, 18, 31, 32, 33, then one track with a grossly wrong observation, one whose point lies 1e12 away (parallel rays), and
    ragged lengths 2 .. 40.  Observations carry pixel noise, so the refinement has work to do."""
    rng = np.random.default_rng(seed)
    cam_model, cam_params = _table(("perspective", "brown"))
    centres = np.c_[np.arange(N_STREET) * 0.05, rng.normal(0, 0.02, N_STREET), rng.normal(0, 0.02, N_STREET)]
    shot_pose = np.array([_pose_row(rng.normal(0, 0.02, 3), centres[s]) for s in range(N_STREET)])
    shot_camera = (np.arange(N_STREET) % 2).astype(np.int32)
    fixed = list(LENGTHS) + [15, 16, 17, 18, 31, 32, 33]
    obs_shot, obs_xy, lengths, points = [], [], [], []
    for t in range(n_tracks):
        gross = t == len(fixed)
        far = t == len(fixed) + 1
        L = fixed[t] if t < len(fixed) else 5 if gross else 3 if far else int(round(math.exp(rng.uniform(math.log(2), math.log(40)))))
        stride = 1 if L > 40 else 6 if t < len(fixed) else int(rng.integers(1, 7))  # (a wide baseline for the boundary lengths: they triangulate)
        first = int(rng.integers(0, N_STREET - max(L - 1, 0) * stride))
        X = np.array([centres[first + (L // 2) * stride, 0] + rng.uniform(-0.3, 0.3), rng.uniform(-1.0, 1.0),
                      rng.uniform(12.0, 16.0) if L > 100 else rng.uniform(6.0, 9.0) if stride > 1 else rng.uniform(4.0, 9.0)])
        if far:
            X[2] = 1e12
        for k in range(L):
            s = first + k * stride
            u, v = _project(int(cam_model[shot_camera[s]]), cam_params[shot_camera[s]], shot_pose[s], X)
            noise = rng.normal(0, 3e-4, 2)
            if gross and k == 2:
                noise = np.array([0.05, -0.04])
            obs_shot.append(s)
            obs_xy.append([u + noise[0], v + noise[1]])
        lengths.append(L)
        points.append(X)
    return {"params": DEFAULT, "offsets": np.r_[0, np.cumsum(lengths)].astype(np.int64), "shot_pose": shot_pose, "shot_camera": shot_camera,
            "cam_model": cam_model, "cam_params": cam_params, "obs_shot": np.array(obs_shot, np.int32).reshape(-1),
            "obs_xy": np.array(obs_xy, np.float64).reshape(-1, 2), "approximate": np.array(points)}


@functools.lru_cache(maxsize=None)
def model_scene(model, n_tracks=48, n_shots=30, seed=21):
    """every shot uses `model`; tracks of 2 .. 12 shots around a street, pixel noise"""
    rng = np.random.default_rng(seed + MODELS.index(model))
    cam_model, cam_params = _table((model,))
    centres = np.c_[np.arange(n_shots) * 0.3, rng.normal(0, 0.05, n_shots), rng.normal(0, 0.05, n_shots)]
    shot_pose = np.array([_pose_row(rng.normal(0, 0.03, 3), centres[s]) for s in range(n_shots)])
    obs_shot, obs_xy, lengths = [], [], []
    for t in range(n_tracks):
        L = int(rng.integers(2, 13))
        first = int(rng.integers(0, n_shots - L + 1))
        X = [centres[first + L // 2, 0] + rng.uniform(-0.5, 0.5), rng.uniform(0.2, 1.2) * (1 if t % 2 else -1), rng.uniform(4.0, 9.0)]
        for s in range(first, first + L):
            u, v = _project(int(cam_model[0]), cam_params[0], shot_pose[s], X)
            obs_shot.append(s)
            obs_xy.append([u + rng.normal(0, 3e-4), v + rng.normal(0, 3e-4)])
        lengths.append(L)
    return {"params": DEFAULT, "offsets": np.r_[0, np.cumsum(lengths)].astype(np.int64), "shot_pose": shot_pose,
            "shot_camera": np.zeros(n_shots, np.int32), "cam_model": cam_model, "cam_params": cam_params,
            "obs_shot": np.array(obs_shot, np.int32), "obs_xy": np.array(obs_xy, np.float64)}


def _unit(x):
    x = np.asarray(x, float)
    return x / np.linalg.norm(x)


@functools.lru_cache(maxsize=None)
def special_scene():
    """one track per special case, as rays; the expected statuses are SPECIAL_STATUS"""
    a = math.radians(0.5)
    tracks = [
        ([[0, 0, 0], [1, 0, 0], [2, 0, 0]], [[0, 0, 1.0]] * 3),                                        # parallel rays: 2
        ([[0, 0, 0], [0, 0, 10.0]], [[math.sin(a / 2), 0, math.cos(a / 2)], [math.sin(a / 2), 0, -math.cos(a / 2)]]),  # 179.5 degrees apart: 2
        ([[0, 0, 0], [0, 0, 0]], [_unit([0.0, 0, 1]), _unit([-1.0, 0, 1])]),                            # coincident origins: 4
        # the rays meet at (0, 0, 2), behind both cameras.  A point behind a camera has a reprojection angle of ~pi and fails THAT test
        # first -- unless the cosine is <= -1 exactly, where AngleBetweenVectors returns 0: the first ray is (0, 0, -1) from the origin,
        # so its cosine is -2 / sqrt(4 + dx^2) = -1 for any rounding dx of the midpoint, and the track reaches the depth test: 4
        ([[0, 0, 0], [1, 0, 0]], [[0.0, 0.0, -1.0], -_unit([-1.0, 0, 2])]),
        ([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]],
         [_unit([1.5, 0.2, 5]), _unit([0.5, 0.2, 5]), _unit([-0.5, 0.2, 5]), _unit([-1.5, 0.6, 5])]),  # one gross observation: 3
        ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [_unit([0.5, 0.4, 5]), _unit([-0.5, 0.4, 5]), _unit([0.5, -0.6, 5])]),  # a good one: 0
    ]
    return {"params": DEFAULT, "offsets": np.r_[0, np.cumsum([len(o) for o, _ in tracks])].astype(np.int64),
            "centers": np.array([r for o, _ in tracks for r in o], np.float64), "bearings": np.array([r for _, w in tracks for r in w], np.float64)}


SPECIAL_STATUS = [2, 2, 4, 4, 3, 0]


def _spherical_pair(translation2, min_depth):
    """the TrackTriangulator cases of the reference's test_triangulation.py: two spherical shots, observations (0, 0) and (-0.1, 0)"""
    cam_model, cam_params = _table(("spherical",))
    shot_pose = np.array([np.r_[np.eye(3).reshape(9), [0.0, 0.0, 0.0]], np.r_[np.eye(3).reshape(9), translation2]])
    return {"params": dict(REFERENCE, min_depth=min_depth), "offsets": np.array([0, 2], np.int64), "shot_pose": shot_pose,
            "shot_camera": np.zeros(2, np.int32), "cam_model": cam_model, "cam_params": cam_params, "obs_shot": np.array([0, 1], np.int32),
            "obs_xy": np.array([[0.0, 0.0], [-0.1, 0.0]])}


def reference_spherical_scene():
    return _spherical_pair([-1.0, 0.0, 0.0], 0.001)  # expects [0, 0, 1.3763819204711]


def reference_coincident_scene():
    return _spherical_pair([0.0, 0.0, 0.0], 0.0001)  # expects no point: depth


def reference_midpoint_scene():
    """the midpoint literals of the same file: X = [0, 0, 1], and coincident origins"""
    b1, b2 = _unit([0.0, 0, 1]), _unit([-1.0, 0, 1])
    return {"params": REFERENCE, "offsets": np.array([0, 2, 4], np.int64), "centers": np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0], [0.0, 0, 0]]),
            "bearings": np.array([b1, b2, b1, b2])}


@functools.lru_cache(maxsize=None)
def ray_scene(noise, n_tracks=64, seed=31):
    """rays towards known points from cameras spread widely around them (angles of tens of degrees), lengths 2 .. 40; `noise` radians of
    direction noise (0: the rays meet in "truth" exactly up to the rounding of one normalisation)"""
    rng = np.random.default_rng(seed)
    centers, bearings, lengths, truth = [], [], [], []
    for t in range(n_tracks):
        L = (2, 3, 8, 9, 16, 17, 40)[t] if t < 7 else int(round(math.exp(rng.uniform(math.log(2), math.log(40)))))
        X = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(6.0, 12.0)])
        o = np.c_[rng.uniform(-4, 4, L), rng.uniform(-4, 4, L), rng.uniform(-1, 1, L)]
        o[0, :2], o[1, :2] = [-3.0, -2.0], [3.0, 2.0]  # never a narrow pair only
        d = X[None, :] - o
        d = d / np.linalg.norm(d, axis=1)[:, None]
        if noise:
            d = d + rng.normal(0, noise, d.shape)
            d = d / np.linalg.norm(d, axis=1)[:, None]
        centers.append(o)
        bearings.append(d)
        lengths.append(L)
        truth.append(X)
    # (noise of 0.01 and more would fail the default reprojection threshold: those scenes run with a loose one, and their first steps
    # change the cost by more than TinySolver's 1e-6, so the solver goes on for several iterations)
    return {"params": DEFAULT if noise < 0.01 else dict(DEFAULT, threshold=0.3), "offsets": np.r_[0, np.cumsum(lengths)].astype(np.int64),
            "centers": np.concatenate(centers), "bearings": np.concatenate(bearings), "truth": np.array(truth)}


def rays_of(scene):
    if "centers" in scene:
        return scene["centers"], scene["bearings"]
    return world_rays(scene)


def restatement(scene):
    """every track of a scene through restate_track -> {"points", "status", "iterations", "borderline"}"""
    o, w = rays_of(scene)
    off = scene["offsets"]
    n = len(off) - 1
    points, status, iterations, hanging = np.full((n, 3), np.nan), np.zeros(n, np.uint8), np.zeros(n, np.int32), []
    for t in range(n):
        st, X, it, notes = restate_track(o[off[t]:off[t + 1]], w[off[t]:off[t + 1]], scene["params"])
        points[t], status[t], iterations[t] = X, st, it
        hanging += [(t,) + note for note in borderline_notes(notes)]
    return {"points": points, "status": status, "iterations": iterations, "borderline": hanging}


def borderline(ref):
    return ref["borderline"]


_SCENES = {"special": special_scene, "ref_spherical": reference_spherical_scene, "ref_coincident": reference_coincident_scene,
           "ref_midpoint": reference_midpoint_scene}


@functools.lru_cache(maxsize=None)
def scene(kind, arg=None):
    if kind == "ragged":
        return ragged_scene(arg)
    if kind == "model":
        return model_scene(arg)
    if kind == "rays":
        return ray_scene(arg)
    if kind == "rig":
        return rig_scene()
    return _SCENES[kind]()


@functools.lru_cache(maxsize=None)
def reference(kind, arg=None):
    """the restatement of a scene, computed once per session and shared"""
    return restatement(scene(kind, arg))


ALL_SCENES = ([("ragged", n) for n in (1, 63, 64, 65, 3000)] + [("model", m) for m in MODELS] +
              [("rig", None), ("special", None), ("ref_spherical", None), ("ref_coincident", None), ("ref_midpoint", None), ("rays", 0.0), ("rays", 1e-3), ("rays", 0.03)])
EMULATED_SCENES = ALL_SCENES  # (the 3 000 tracks take the host emulation ~7 s per entry point)


# ---------------------------------------------------------------------------------------------------------------------------------
# a reconstruction with rigs and two camera models, and a tracks manager over it
# ---------------------------------------------------------------------------------------------------------------------------------
def rig_reconstruction():
    """geometry_types objects of a ``synthetic.make_bundle_scene`` problem (rigs, perspective + brown, ground-truth cameras and poses,
    noisy observations of which 3 % are grossly wrong) with every observation in a TracksManager and no point in the map yet; the
    manager also knows a shot the reconstruction does not hold and a track with one observation -> (reconstruction, manager)"""
    from opensfm_amd import synthetic
    from opensfm_amd.geometry_types import (Camera, Observation, Pose, Reconstruction, RigCamera, RigInstance, TracksManager,
                                            set_camera_parameter_values)

    models = ("perspective", "brown")
    prob = synthetic.make_bundle_scene(models=models, seed=3, n_gcp=0, up_vectors=False, free_bias=False)
    r = Reconstruction()
    for c, m in enumerate(models):
        cam = Camera(m)
        set_camera_parameter_values(cam, prob["gt_cam"][c])
        cam.id = "c%d" % c
        r.add_camera(cam)
    for k, v in enumerate(prob["gt_rig_camera"]):
        r.add_rig_camera(RigCamera("rc%d" % k, Pose.from_cam_to_world(v[:3], v[3:])))
    for k, v in enumerate(prob["gt_rig_instance"]):
        r.add_rig_instance(RigInstance("i%d" % k, Pose.from_cam_to_world(v[:3], v[3:])))
    for s in range(len(prob["shot_camera"])):
        r.create_shot("s%03d" % s, "c%d" % prob["shot_camera"][s], None, "rc%d" % prob["shot_rig_camera"][s], "i%d" % prob["shot_rig_instance"][s])
    manager = TracksManager()
    for s, p, xy, sd in zip(prob["obs_shot"], prob["obs_point"], prob["obs_xy"], prob["obs_sigma"]):
        manager.add_observation("s%03d" % s, "p%d" % p, Observation(xy[0], xy[1], sd))
    for k in range(40):
        manager.add_observation("ghost", "p%d" % k, Observation(0.01 * k, -0.02, 0.004))
    manager.add_observation("s000", "lonely", Observation(0.1, 0.1, 0.004))
    return r, manager


def _flatten(r, manager, track_ids):
    """the pixel scene of `track_ids`, straight from the objects: shots in map order, observations in the manager's order"""
    shot_ids = list(r.shots)
    cam_ids = list(r.cameras)
    cam_params = np.zeros((len(cam_ids), 16))
    for c, cid in enumerate(cam_ids):
        v = r.cameras[cid].get_parameters_values()
        cam_params[c, :len(v)] = v
    shot_pose = np.array([np.r_[r.shots[s].pose.get_R_world_to_cam().reshape(9), r.shots[s].pose.get_t_world_to_cam()] for s in shot_ids])
    obs_shot, obs_xy, lengths, members = [], [], [], []
    for t in track_ids:
        ids = [s for s in manager.get_track_observations(t) if s in r.shots]
        obs_shot += [shot_ids.index(s) for s in ids]
        obs_xy += [manager.get_observation(s, t).point for s in ids]
        lengths.append(len(ids))
        members.append(ids)
    flat = {"params": DEFAULT, "offsets": np.r_[0, np.cumsum(lengths)].astype(np.int64), "shot_pose": shot_pose,
            "shot_camera": np.array([cam_ids.index(r.shots[s].camera.id) for s in shot_ids], np.int32),
            "cam_model": np.array([MODELS.index(r.cameras[c].projection_type) for c in cam_ids], np.int32), "cam_params": cam_params,
            "obs_shot": np.array(obs_shot, np.int32), "obs_xy": np.array(obs_xy, np.float64).reshape(-1, 2)}
    return flat, members


@functools.lru_cache(maxsize=None)
def rig_scene():
    r, manager = rig_reconstruction()
    return _flatten(r, manager, manager.get_track_ids())[0]


def expected_map(r, manager, track_ids, params=DEFAULT):
    """a per-track Python loop over the restatement: {track id: (coordinates, set of observing shots)} of the accepted tracks"""
    flat, members = _flatten(r, manager, track_ids)
    flat["params"] = params
    ref = restatement(flat)
    assert len(ref["borderline"]) == 0
    return {t: (ref["points"][k], set(members[k])) for k, t in enumerate(track_ids) if ref["status"][k] == 0}


# ---------------------------------------------------------------------------------------------------------------------------------
# running and comparing (shared by tests/test_triangulate_host.py and tests/test_gpu_triangulate.py)
# ---------------------------------------------------------------------------------------------------------------------------------
# Largest relative difference (|X - X_ref| / |X_ref|) between triangulate.hip on the host emulation and restate_track over EMULATED_SCENES,
# measured on the CPU: MEASURED_POINT_DIFFERENCE.  Both are float64 evaluations of the same step sequence and differ in summation
# order only; the tolerance is 100 x that.
MEASURED_POINT_DIFFERENCE = 6.9e-14  # (6.8e-14, in the 3 000-track ragged scene; 3e-15 and less in the others)
POINT_RTOL = 100 * MEASURED_POINT_DIFFERENCE
# Largest relative distance between restate_track (10 iterations) and the 50-digit minimiser over ray_scene(1e-3) and ray_scene(0.03): TinySolver's absolute
# 1e-6 cost-change stop ends these tracks after their first accepted step (noise 1e-3) or their second (noise 0.03).  The bound is 10 x that.
MEASURED_MINIMISER_DISTANCE = 1.1e-5  # (1.09e-5)
MINIMISER_RTOL = 10 * MEASURED_MINIMISER_DISTANCE


def run_tracks(sc, ctx=None):
    from opensfm_amd import reconstruction

    p = sc["params"]
    return reconstruction.triangulate_tracks_arrays(sc["shot_pose"], sc["shot_camera"], sc["cam_model"], sc["cam_params"], sc["obs_shot"], sc["obs_xy"],
                                                    sc["offsets"], p["threshold"], p["min_angle_deg"], p["min_depth"], p["iterations"], ctx=ctx)


def run_bearings(sc, ctx=None):
    from opensfm_amd import reconstruction

    o, w = rays_of(sc)
    p = sc["params"]
    return reconstruction.triangulate_bearings_arrays(o, w, sc["offsets"], p["threshold"], p["min_angle_deg"], p["min_depth"], p["iterations"], ctx=ctx)


def relative_difference(a, b):
    """largest |a_t - b_t| / |b_t| over the tracks where b is a point"""
    ok = ~np.isnan(b).any(axis=1)
    if not ok.any():
        return 0.0
    return float((np.linalg.norm(a[ok] - b[ok], axis=1) / np.linalg.norm(b[ok], axis=1)).max())


def check(got, ref, rtol=None):
    """identical statuses and iteration counts (the scene has no borderline comparison), NaN exactly where rejected, points within rtol;
    returns the largest relative difference"""
    rtol = POINT_RTOL if rtol is None else rtol
    points, status, iterations = got[0], got[1], got[2]
    assert len(ref["borderline"]) == 0, ref["borderline"][:5]
    diff = relative_difference(points, ref["points"])
    print("largest relative point difference %.3g over %d points (tolerance %.3g)" % (diff, int((ref["status"] == 0).sum()), rtol))
    assert np.array_equal(status, ref["status"])
    assert np.array_equal(iterations, ref["iterations"])
    assert np.array_equal(np.isnan(points).any(axis=1), ref["status"] != 0) and np.array_equal(np.isnan(points).all(axis=1), ref["status"] != 0)
    assert diff <= rtol
    return diff
