"""Scenes on which the Levenberg-Marquardt driver of opensfm_amd/csrc/ba.hip has to take its way back: the CPU oracle rejects steps on them
(two in a row, with accepted steps after them), so the speculative linearisation of the candidate is undone -- blocks swapped back, the old
point linearised again -- and the next iteration starts from device state that a rejection has been through.  Next to them the degenerate
free sets (an empty reduced system, a border-only system, nothing free at all).  Shared by tests/test_ba_recovery_premises.py (CPU: the
oracle alone must show the recorded rejections, away from the acceptance threshold), tests/test_gpu_ba_recovery.py and tests/test_emu_ba.py.

An iteration i is rejected when cost_history[i] == cost_history[i - 1]: a rejected step leaves the cost where it was, bit for bit, and an
accepted one has rho > 1e-3, that is a cost that went down.  The lists below are the oracle's, recorded once; the premises test keeps them true."""
import numpy as np

from opensfm_amd import synthetic

NO_TOL = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
PX = 2000.0  # max(w, h) of the synthetic camera: normalized -> pixels
NOISY = dict(pose_noise_t=0.5, pose_noise_r=0.1, point_noise=0.5, outlier_frac=0.2)
RHO_ACCEPT = 1e-3  # ceres' min_relative_decrease, the threshold of both oracles and of trust_region_step
RHO_MARGIN = 5e-3  # no oracle decision may sit closer to it than this: the GPU tests do not pass on a coin flip


def _narrow20():
    return synthetic.make_ba_scene(20, 300, 5, seed=12, **NOISY)


def _wide40():
    return synthetic.make_ba_scene(40, 800, 12, seed=15, pose_noise_t=0.5, pose_noise_r=0.1, point_noise=0.5)


def _local30():
    from opensfm_amd import bundle

    pr = synthetic.make_ba_scene(30, 450, 6, seed=12, **NOISY)
    return bundle.local_problem(pr, 15, {"local_bundle_radius": 3, "local_bundle_min_common_points": 10, "local_bundle_max_shots": 30})[0]


def _s1025():
    return synthetic.make_ba_scene(1025, 4100, 4, seed=5, **NOISY)


def _grid6x14():
    return synthetic.make_ba_scene_grid(6, 14, 1200, 9, seed=5, pose_noise_t=1.0, pose_noise_r=0.2, point_noise=1.0, outlier_frac=0.3)


def _generic(model, outlier_frac, sd_points, sd_poses):
    pr = synthetic.make_bundle_scene(models=(model,), n_instances=8, n_points=100, rig=False, gps=False, n_gcp=0, up_vectors=False, seed=7,
                                     outlier_frac=outlier_frac)
    rng = np.random.default_rng(107)  # the points first, then the poses
    pr["points"] = pr["points"] + rng.normal(0, sd_points, pr["points"].shape)
    pr["rig_instance_pose"] = pr["rig_instance_pose"] + rng.normal(0, sd_poses, pr["rig_instance_pose"].shape)
    return pr


# name -> (builder, solver, loss, LM iterations, the oracle's rejected iterations)
#   solver "ba": osfm_ba_solve / oracle.ba_solve ([k1 k2 focal] kernels); "general": osfm_bundle_solve / oracle.bundle_general (generic rows)
SCENES = {
    "narrow20": (_narrow20, "ba", "TrivialLoss", 12, [4, 5, 7, 10]),
    "wide40": (_wide40, "ba", "CauchyLoss", 12, [6, 7, 9]),  # half-width 11: the wide band
    "local30": (_local30, "ba", "TrivialLoss", 12, [5, 6, 7]),  # 21 free shots, constant cameras
    "s1025": (_s1025, "ba", "TrivialLoss", 10, [2, 3, 4]),  # rho down to -6.9e18: candidate costs near 1e22
    "grid6x14": (_grid6x14, "ba", "CauchyLoss", 12, [3, 9, 10]),
    "gen_spherical": (lambda: _generic("spherical", 0.3, 1.0, 0.2), "general", "TrivialLoss", 12, [3, 4]),
    # nine free intrinsics in the border.  (Standard deviations 0.6 / 0.12 had been proposed for this scene: the oracle has converged to rounding
    #  by iteration 10 there -- 734.2684747 from then on -- and rejects every later step, 11 .. 21, on a cost change of a few ulps: no accepted
    #  step follows and the decisions are noise.  At 1.2 / 0.24 the rejections come while the cost still falls by half per step.)
    "gen_brown": (lambda: _generic("brown", 0.2, 1.2, 0.24), "general", "TrivialLoss", 12, [1, 2, 4, 5, 6, 7, 8]),  # five in a row, then four steps
}

_PROBLEMS = {}
_ORACLE = {}


def problem(name):
    """the scene, built once; nobody modifies it (the solvers copy their inputs)"""
    if name not in _PROBLEMS:
        _PROBLEMS[name] = SCENES[name][0]()
    return _PROBLEMS[name]


def solver(name):
    return SCENES[name][1]


def config(name):
    _, _, loss, iters, _ = SCENES[name]
    return {"loss_function": loss, "loss_function_threshold": 1.0, "bundle_max_iterations": iters}


def recorded(name):
    return list(SCENES[name][4])


def oracle_solve(oracle_lib, name, verbose=False):
    """the oracle's solve of a scene, once per session (the verbose run is not cached: its output is the point)"""
    _, kind, loss, iters, _ = SCENES[name]
    if kind == "general":
        run = lambda: oracle_lib.bundle_general(problem(name), loss=loss, max_iterations=iters, **NO_TOL)
    else:
        run = lambda: oracle_lib.ba_solve(problem(name), loss=loss, max_iterations=iters, verbose=verbose, **NO_TOL)
    if verbose:
        return run()
    if name not in _ORACLE:
        _ORACLE[name] = run()
    return _ORACLE[name]


def rejected(cost_history, n=None):
    """the iterations 1 .. n whose step was not taken: the cost stayed where it was, bit for bit"""
    h = np.asarray(cost_history, float)
    n = len(h) - 1 if n is None else n
    return [i for i in range(1, n + 1) if h[i] == h[i - 1]]


def first_run_of_rejections(rej):
    """(first, last) of the first run of at least two consecutive rejected iterations, or None"""
    for i, a in enumerate(rej):
        j = i
        while j + 1 < len(rej) and rej[j + 1] == rej[j] + 1:
            j += 1
        if j > i:
            return a, rej[j]
    return None


def rmse_px(err):
    e = np.asarray(err, float)[:, :2]
    return float(np.sqrt((e**2).sum(1).mean()) * PX)


def max_rel_cost_diff(g, o):
    a, b = np.asarray(g["cost_history"], float), np.asarray(o["cost_history"], float)
    return float(np.max(np.abs(a - b) / np.abs(b))) if len(a) == len(b) and len(a) else float("inf")


def check_against_oracle(g, o):
    """the device walked the oracle's trajectory, rejections included: same counts, the same iterations rejected, cost history to 1e-7
    relative (the figure of test_gpu_ba.py::test_lm_trajectory_equals_oracle), final reprojection RMSE within 1e-4 px (north star)"""
    print("rejected: device %s oracle %s; max relative cost-history difference %.3e; rmse %.9f / %.9f px"
          % (rejected(g["cost_history"]), rejected(o["cost_history"]), max_rel_cost_diff(g, o), rmse_px(g["reproj_err"]), rmse_px(o["reproj_err"])))
    assert g["iterations"] == o["iterations"], (g["iterations"], o["iterations"])
    assert g["successful_steps"] == o["successful_steps"], (g["successful_steps"], o["successful_steps"])
    assert rejected(g["cost_history"]) == rejected(o["cost_history"])
    assert np.allclose(g["cost_history"], o["cost_history"], rtol=1e-7, atol=0), (g["cost_history"], o["cost_history"])
    assert abs(rmse_px(g["reproj_err"]) - rmse_px(o["reproj_err"])) < 1e-4


# ---- degenerate free sets -------------------------------------------------------------------------------------------------------------
# on make_ba_scene(12, 200, 5, seed=4), 8 iterations: which blocks are constant.  "points_only": every shot and camera constant = an empty
# reduced system; "camera_only": the border alone; "nothing": no variable at all (0 iterations, termination 2: the gradient over no variable
# is 0 <= any tolerance)
DEGENERATE_ITERATIONS = 8


def degenerate_base():
    if "degenerate" not in _PROBLEMS:
        _PROBLEMS["degenerate"] = synthetic.make_ba_scene(12, 200, 5, seed=4)
    return _PROBLEMS["degenerate"]


def _one_free(n, k):
    f = np.ones(n, np.uint8)
    f[k] = 0
    return f


# name -> (cameras constant, shots constant, points constant) as functions of the block count
DEGENERATE_SETS = {
    "points_only": (lambda n: np.ones(n, np.uint8), lambda n: np.ones(n, np.uint8), lambda n: np.zeros(n, np.uint8)),
    "camera_only": (lambda n: np.zeros(n, np.uint8), lambda n: np.ones(n, np.uint8), lambda n: np.ones(n, np.uint8)),
    "shots_only": (lambda n: np.ones(n, np.uint8), lambda n: np.zeros(n, np.uint8), lambda n: np.ones(n, np.uint8)),
    "nothing": (lambda n: np.ones(n, np.uint8), lambda n: np.ones(n, np.uint8), lambda n: np.ones(n, np.uint8)),
    "one_shot": (lambda n: np.ones(n, np.uint8), lambda n: _one_free(n, 5), lambda n: np.zeros(n, np.uint8)),
    "one_point": (lambda n: np.ones(n, np.uint8), lambda n: np.ones(n, np.uint8), lambda n: _one_free(n, 17)),
}


def degenerate_problem(name, general=False):
    """the flat problem with the set's constant flags -- or its general layout (tests/test_oracle_bundle_general._as_general) with them"""
    cam, shot, point = DEGENERATE_SETS[name]
    pr = dict(degenerate_base())
    pr["cam_fixed"] = cam(len(pr["cam_params"]))
    pr["shot_fixed"] = shot(len(pr["shot_pose"]))
    pr["point_fixed"] = point(len(pr["points"]))
    if not general:
        return pr
    import test_oracle_bundle_general as og

    g = og._as_general(pr)
    g["rig_instance_fixed"] = pr["shot_fixed"]
    g["point_fixed"] = pr["point_fixed"]
    return g
