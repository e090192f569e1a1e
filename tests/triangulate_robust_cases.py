"""Scenes and a numpy restatement for the robust track triangulation of ``opensfm_amd/csrc/triangulate.hip``
(``osfm_triangulate_bearings_robust`` / ``osfm_triangulate_tracks_robust``), written from the text of ``opensfm/reconstruction.py:922-1030``
(``TrackTriangulator.triangulate_robust``).

``restate_track_robust`` follows the walk step by step in float64 over the pieces of ``triangulate_cases`` (the two-row solve is its
``restate_track``: the pair test, ``midpoint``, the two per-row tests, ``refine``; the subset refinement is ``refine``), with ``math.log``
for the stopping rule.  It keeps every comparison it makes as a note, so that ``borderline`` can say whether a decision hung on rounding,
and a log of the branch every try took.  ``draw`` restates the library's generator with Python integers.

Every scene here is chosen so that its ``borderline`` list is empty (checked by the CPU tests with the restatement alone); status,
inlier_mask, n_inliers and tries_used of the kernels must then be identical to the restatement's."""
import functools
import math

import numpy as np

import triangulate_cases as base
from triangulate_cases import BORDERLINE, DEFAULT, angle_between, midpoint, refine  # noqa: F401  (the pieces the walk is made of)

TRIES = 11
MASK64 = (1 << 64) - 1


def draw(seed, t, k):
    """draw k of track t: splitmix64's finaliser over seed + 0x9E3779B97F4A7C15 (11 t + k + 1), the top 53 bits times 2^-53"""
    z = (seed + 0x9E3779B97F4A7C15 * (11 * t + k + 1)) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return (z >> 11) * 2.0 ** -53


def seeded_draws(seed, n_tracks):
    return np.array([[draw(seed, t, k) for k in range(TRIES)] for t in range(n_tracks)], np.float64).reshape(n_tracks, TRIES)


def unrank(rank, n):
    """the pair (i < j) of lexicographic rank `rank` among the pairs of n, by walking the rows"""
    i = 0
    while rank >= n - 1 - i:
        rank -= n - 1 - i
        i += 1
    return i, i + 1 + rank


def chords(o, w, X):
    """|(X - o_k) / |X - o_k| - w_k|, as the reference writes it"""
    with np.errstate(all="ignore"):
        r = X[None, :] - o
        r = r / np.linalg.norm(r, axis=1)[:, np.newaxis]
        return np.linalg.norm(r - w, axis=1)


def restate_track_robust(o, w, draws, prm=DEFAULT):
    """-> {"status", "point" (NaN unless 0), "mask" (n,) uint8, "n_inliers", "tries", "notes", "log" (one word per try made)}"""
    o = np.asarray(o, np.float64).reshape(-1, 3)
    w = np.asarray(w, np.float64).reshape(-1, 3)
    n = len(o)
    out = {"status": 1, "point": np.full(3, np.nan), "mask": np.zeros(n, np.uint8), "n_inliers": 0, "tries": 0, "notes": [], "log": []}
    if n < 2:
        return out
    notes, log = out["notes"], out["log"]
    threshold = prm["threshold"]
    C = n * (n - 1) // 2
    best_inliers, best_point, tried = np.zeros(0, np.int64), None, set()
    for attempt in range(TRIES):
        out["tries"] = attempt + 1
        random_id = int(float(draws[attempt]) * (C - 1))
        if random_id in tried:
            log.append("repeat")
            continue
        i, j = unrank(random_id, n)
        tried.add(random_id)
        status, X, _, pair_notes = base.restate_track(o[[i, j]], w[[i, j]], prm)
        notes += pair_notes
        if status != 0:
            log.append("invalid")
            continue
        d = chords(o, w, X)
        notes += [("chord", v, threshold) for v in d]
        inliers = np.flatnonzero(d < threshold)
        if not len(inliers) > len(best_inliers):
            log.append("not better")
            continue
        new_X, _ = refine(o[inliers], w[inliers], X, prm["iterations"], notes)  # (from X: the midpoint over the inliers is dead code)
        d = chords(o, w, new_X)
        notes += [("chord", v, threshold) for v in d]
        ls_inliers = np.flatnonzero(d < threshold)
        if len(ls_inliers) > len(inliers):
            best_inliers, best_point, word = ls_inliers, new_X, "ls wins"
        else:
            best_inliers, best_point, word = inliers, X, "ls loses"
        ratio = float(len(best_inliers)) / n
        if ratio == 1.0:
            log.append(word + ", all inliers")
            break
        optimal_iter = math.log(1.0 - 0.99) / math.log(1.0 - ratio * ratio)
        notes.append(("optimal_iter", optimal_iter, float(i)))
        if optimal_iter <= i:  # (i: the first index of the sampled pair)
            log.append(word + ", enough")
            break
        log.append(word + ", goes on")
    if len(best_inliers) > 1:
        if not np.isfinite(best_point).all():
            out["status"] = 5
            return out
        out["status"], out["point"], out["n_inliers"] = 0, np.array(best_point), len(best_inliers)
        out["mask"][best_inliers] = 1
    else:
        out["status"] = 6
    return out


def borderline_notes(notes):
    """triangulate_cases' rule, with a bound of 0 (optimal_iter <= 0) compared absolutely"""
    out = base.borderline_notes([x for x in notes if x[2] != 0.0 or x[0] == "rho"])
    return out + [x for x in notes if x[0] != "rho" and x[2] == 0.0 and abs(x[1]) <= BORDERLINE]


def restatement(scene, draws):
    """every track of a scene with its row of `draws` -> {"points", "status", "mask", "n_inliers", "tries", "borderline", "log"}"""
    o, w = base.rays_of(scene)
    off = scene["offsets"]
    n = len(off) - 1
    ref = {"points": np.full((n, 3), np.nan), "status": np.zeros(n, np.uint8), "mask": np.zeros(len(o), np.uint8),
           "n_inliers": np.zeros(n, np.int32), "tries": np.zeros(n, np.int32), "borderline": [], "log": []}
    for t in range(n):
        r = restate_track_robust(o[off[t]:off[t + 1]], w[off[t]:off[t + 1]], draws[t], scene["params"])
        ref["points"][t], ref["status"][t], ref["n_inliers"][t], ref["tries"][t] = r["point"], r["status"], r["n_inliers"], r["tries"]
        ref["mask"][off[t]:off[t + 1]] = r["mask"]
        ref["borderline"] += [(t,) + note for note in borderline_notes(r["notes"])]
        ref["log"].append(r["log"])
    return ref


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 3, 4, 8, 9, 31, 32, 33, 63, 64, 65, 513, 600)  # C = 1 and 3, the lane-group split, the wavefront, past kWaveObs
N_RAYS = 300
SEED = 2026  # of the library's generator, where a test does not give the draws
# seeds of the scenes and of the explicit draws: chosen so that no scene has a borderline comparison (test_no_scene_has_a_borderline_comparison)
RAY_SEED, PIXEL_SEED, DRAWS_SEED = 28, 3, 77
NOISY_SEED = 0
NOISY_DRAWS = (0.5,) * 11


def _track(rng, L, outlier_fraction, noise):
    """L rays towards one point from cameras spread around it, `noise` radians of direction noise; a fraction of them gross outliers"""
    X = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(6.0, 12.0)])
    o = np.c_[rng.uniform(-4, 4, L), rng.uniform(-4, 4, L), rng.uniform(-1, 1, L)]
    d = X[None, :] - o
    d = d / np.linalg.norm(d, axis=1)[:, None] + rng.normal(0, noise, (L, 3))
    wrong = rng.permutation(L)[:int(round(outlier_fraction * L))]
    d[wrong] += rng.normal(0, 0.3, (len(wrong), 3))
    return o, d / np.linalg.norm(d, axis=1)[:, None], X


def _noise(L):
    """Direction noise of a track's good rays, radians.  A sample whose inliers are the two sampled rows alone is refined twice over
    the same rows, and the second run starts one step from the optimum: at 1e-3 its first step changes the cost by ~1e-10 of the cost,
    which triangulate_cases counts as borderline (the sign of rho).  At 1e-5 the second run finds its gradient below TinySolver's 1e-10
    and returns at once.  Short tracks, where that is the usual sample, get the small noise; the long ones noise of the threshold's
    order, so that the subset refinement changes the inlier set."""
    return 1e-5 if L < 8 else 1e-3 if L % 2 else 2e-3


@functools.lru_cache(maxsize=None)
def ray_scene(seed=RAY_SEED):
    """300 tracks as rays: the lengths of LENGTHS first, then LENGTHS' long ones again with other outlier shares, then ragged 2 .. 40;
    0 - 60 % gross outlier rays, _noise() on the rest (the threshold is 0.006)"""
    rng = np.random.default_rng(seed)
    lengths = list(LENGTHS) + [64, 65, 513, 600, 33, 32]
    centers, bearings, sizes, truth = [], [], [], []
    for t in range(N_RAYS):
        L = lengths[t] if t < len(lengths) else int(round(math.exp(rng.uniform(math.log(2), math.log(40)))))
        share = (0.0, 0.1, 0.3, 0.45, 0.6)[t % 5] if t >= len(LENGTHS) else 0.25
        o, w, X = _track(rng, L, share, _noise(L))
        centers.append(o)
        bearings.append(w)
        sizes.append(L)
        truth.append(X)
    return {"params": DEFAULT, "offsets": np.r_[0, np.cumsum(sizes)].astype(np.int64), "centers": np.concatenate(centers),
            "bearings": np.concatenate(bearings), "truth": np.array(truth)}


@functools.lru_cache(maxsize=None)
def pixel_scene(n_tracks=80, seed=PIXEL_SEED):
    """the street, shots and cameras of triangulate_cases.ragged_scene (perspective and brown alternating) under tracks of this module's
    own: a few boundary lengths, then ragged 2 .. 40; pixel noise by _noise() (the points are ~7 away), a fifth of the observations of
    the tracks of 4 and more moved far away: gross mismatches"""
    street = base.ragged_scene(1)
    shot_pose, shot_camera, cam_model, cam_params = street["shot_pose"], street["shot_camera"], street["cam_model"], street["cam_params"]
    rng = np.random.default_rng(seed)
    fixed = [0, 1, 2, 3, 4, 8, 9, 32, 33, 65]
    obs_shot, obs_xy, sizes = [], [], []
    for t in range(n_tracks):
        L = fixed[t] if t < len(fixed) else int(round(math.exp(rng.uniform(math.log(2), math.log(40)))))
        stride = 1 if L > 40 else int(rng.integers(3, 7))
        first = int(rng.integers(0, base.N_STREET - max(L - 1, 0) * stride))
        X = np.array([(first + (L // 2) * stride) * 0.05 + rng.uniform(-0.3, 0.3), rng.uniform(-1.0, 1.0), rng.uniform(6.0, 9.0)])
        wrong = set(rng.permutation(L)[:L // 5].tolist()) if L >= 4 else set()
        for k in range(L):
            s = first + k * stride
            u, v = base._project(int(cam_model[shot_camera[s]]), cam_params[shot_camera[s]], shot_pose[s], X)
            noise = rng.normal(0, _noise(L), 2)
            if k in wrong:
                noise = rng.uniform(0.02, 0.08, 2) * rng.choice([-1.0, 1.0], 2)
            obs_shot.append(s)
            obs_xy.append([u + noise[0], v + noise[1]])
        sizes.append(L)
    return {"params": DEFAULT, "offsets": np.r_[0, np.cumsum(sizes)].astype(np.int64), "shot_pose": shot_pose, "shot_camera": shot_camera,
            "cam_model": cam_model, "cam_params": cam_params, "obs_shot": np.array(obs_shot, np.int32).reshape(-1),
            "obs_xy": np.array(obs_xy, np.float64).reshape(-1, 2)}


def _unit_rows(x):
    x = np.asarray(x, float)
    return x / np.linalg.norm(x, axis=1)[:, None]


# the pair (i, j) of n = 10 has rank i (19 - i) / 2 + j - i - 1 of C = 45; int(u * 44) is the rank
def _u(rank):
    return (rank + 0.5) / 44.0


@functools.lru_cache(maxsize=None)
def forced_scene():
    """Hand-made tracks and draws, one branch each (FORCED names them): 10 rays towards one point with the first three grossly wrong
    (70 % inliers: log(0.01) / log(1 - 0.49) = 6.84), a clean track, a noisy one on which the subset refinement wins, and parallel rays."""
    rng = np.random.default_rng(3)
    o10, w10, _ = _track(rng, 10, 0.0, 0.0)
    w_bad = w10.copy()
    w_bad[:3] = _unit_rows(w_bad[:3] + np.array([[0.2, -0.1, 0.0], [-0.15, 0.2, 0.0], [0.1, 0.25, 0.0]]))
    w_late = w10.copy()  # wrong rows 0, 1 and 8: the last pair, (8, 9), holds one of them
    w_late[[0, 1, 8]] = w_bad[[0, 1, 2]] - w10[[0, 1, 2]] + w10[[0, 1, 8]]
    w_late = _unit_rows(w_late)
    noisy_o, noisy_w, _ = _track(np.random.default_rng(NOISY_SEED), 12, 0.0, 2.5e-3)
    par_o = np.c_[np.arange(5.0), np.zeros(5), np.zeros(5)]
    par_w = np.tile([0.0, 0.0, 1.0], (5, 1))
    rest = [0.31, 0.47, 0.11, 0.83, 0.59, 0.23, 0.71, 0.05, 0.39, 0.93]
    tracks = [
        ("repeated id", o10, w_bad, [_u(24 + 0), _u(24 + 0)] + rest[:9]),            # (3, 4) twice: 6.84 <= 3 fails, then the repeat
        ("all inliers on the first try", o10, w10, [0.5] + rest),
        ("enough by the first index", o10, w_bad, [_u(42)] + rest),                   # (7, 8): 6.84 <= 7
        ("small first index goes on", o10, w_bad, [_u(24 + 1)] + rest),               # (3, 5): 6.84 <= 3 fails
        ("subset refinement wins", noisy_o, noisy_w, list(NOISY_DRAWS)),
        ("subset refinement loses", o10, w_bad, [_u(42 + 1)] + rest),                 # (7, 9)
        ("every try invalid", par_o, par_w, [k / 11.0 for k in range(11)]),
        ("u next to 1", o10, w_late, [1.0 - 2.0 ** -53] + rest),                      # id = C - 2 = 43: (7, 9), never the last pair
    ]
    sizes = [len(o) for _, o, _, _ in tracks]
    return {"params": DEFAULT, "offsets": np.r_[0, np.cumsum(sizes)].astype(np.int64), "centers": np.concatenate([o for _, o, _, _ in tracks]),
            "bearings": np.concatenate([w for _, _, w, _ in tracks]), "draws": np.array([d for _, _, _, d in tracks], np.float64),
            "names": [name for name, _, _, _ in tracks]}


@functools.lru_cache(maxsize=None)
def scene(kind):
    return {"rays": ray_scene, "pixels": pixel_scene, "forced": forced_scene}[kind]()


@functools.lru_cache(maxsize=None)
def draws_of(kind, how):
    """`how`: "explicit" (numpy's generator, or the scene's own hand-made draws) or "seeded" (the library's generator, restated)"""
    sc = scene(kind)
    n = len(sc["offsets"]) - 1
    if how == "seeded":
        return seeded_draws(SEED, n)
    if "draws" in sc:
        return sc["draws"]
    return np.random.default_rng(DRAWS_SEED).random((n, TRIES))


@functools.lru_cache(maxsize=None)
def reference(kind, how):
    """the restatement of a scene, computed once per session and shared"""
    return restatement(scene(kind), draws_of(kind, how))


ALL_RUNS = [("rays", "explicit"), ("rays", "seeded"), ("pixels", "explicit"), ("pixels", "seeded"), ("forced", "explicit")]

# Largest relative difference (|X - X_ref| / |X_ref|) between the robust kernels on the host emulation and restate_track_robust over
# ALL_RUNS and both entry points, measured on the CPU by test_triangulate_robust_host.py.  Both are float64 evaluations of the same
# steps in different summation orders; the tolerance is 100 x that.
MEASURED_POINT_DIFFERENCE = 1.2e-16  # (1.12e-16, in the rays scene with seeded draws: a rounding or two; 6e-17 and less in the others)
POINT_RTOL = 100 * MEASURED_POINT_DIFFERENCE


# ---------------------------------------------------------------------------------------------------------------------------------
# running and comparing (shared by tests/test_triangulate_robust_host.py and tests/test_gpu_triangulate_robust.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def run_bearings(sc, draws=None, seed=0, ctx=None):
    from opensfm_amd import reconstruction

    o, w = base.rays_of(sc)
    p = sc["params"]
    return reconstruction.triangulate_bearings_arrays_robust(o, w, sc["offsets"], p["threshold"], p["min_angle_deg"], p["min_depth"], p["iterations"],
                                                             draws=draws, seed=seed, ctx=ctx)


def run_tracks(sc, draws=None, seed=0, ctx=None):
    from opensfm_amd import reconstruction

    p = sc["params"]
    return reconstruction.triangulate_tracks_arrays_robust(sc["shot_pose"], sc["shot_camera"], sc["cam_model"], sc["cam_params"], sc["obs_shot"],
                                                           sc["obs_xy"], sc["offsets"], p["threshold"], p["min_angle_deg"], p["min_depth"],
                                                           p["iterations"], draws=draws, seed=seed, ctx=ctx)


def run(entry, kind, how, ctx=None):
    """a scene through an entry point: the explicit draws as an array, the seeded ones by the library's own generator"""
    sc = scene(kind)
    fn = run_tracks if entry == "tracks" else run_bearings
    return fn(sc, seed=SEED, ctx=ctx) if how == "seeded" else fn(sc, draws=draws_of(kind, how), ctx=ctx)


def check(got, ref, rtol=None):
    """identical status, mask, n_inliers and tries_used (the scene has no borderline comparison), NaN exactly where there is no point,
    points within rtol; returns the largest relative difference"""
    rtol = POINT_RTOL if rtol is None else rtol
    points, status, mask, n_inliers, tries = got[:5]
    assert len(ref["borderline"]) == 0, ref["borderline"][:5]
    diff = base.relative_difference(points, ref["points"])
    print("largest relative point difference %.3g over %d points (tolerance %.3g), mean tries %.2f" %
          (diff, int((ref["status"] == 0).sum()), rtol, float(ref["tries"].mean()) if len(ref["tries"]) else 0.0))
    assert np.array_equal(status, ref["status"])
    assert np.array_equal(tries, ref["tries"])
    assert np.array_equal(n_inliers, ref["n_inliers"])
    assert np.array_equal(mask, ref["mask"])
    assert np.array_equal(np.isnan(points).any(axis=1), ref["status"] != 0) and np.array_equal(np.isnan(points).all(axis=1), ref["status"] != 0)
    assert diff <= rtol
    return diff


def expected_map(r, manager, track_ids, seed, params=DEFAULT):
    """a per-track Python loop over the restatement with the library's generator: {track id: (coordinates, set of inlier shots)}"""
    flat, members = base._flatten(r, manager, track_ids)
    flat["params"] = params
    ref = restatement(flat, seeded_draws(seed, len(track_ids)))
    assert len(ref["borderline"]) == 0, ref["borderline"][:5]
    off = flat["offsets"]
    return {t: (ref["points"][k], {s for s, m in zip(members[k], ref["mask"][off[k]:off[k + 1]]) if m})
            for k, t in enumerate(track_ids) if ref["status"][k] == 0}
