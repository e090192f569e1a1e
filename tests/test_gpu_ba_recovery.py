"""The way back of the Levenberg-Marquardt driver (opensfm_amd/csrc/ba.hip: lm_loop, straight_line_step, careful_step, candidate_enqueue,
relinearise_old_point) on the device.  The driver is speculative: the candidate is linearised before the host has judged the step, and a
rejected step -- or a straight-line iteration whose single check fails -- is undone by swapping the blocks back and linearising the old
point again.  The scenes of tests/ba_recovery_cases.py make the CPU oracle reject steps, two and more in a row with accepted steps after
them (tests/test_ba_recovery_premises.py holds the oracle to that, and every decision 5e-3 away from the threshold); here the device has
to walk the same trajectory, on every band solver, in generic mode, on a local problem and beyond 1 024 shots; with the straight-line
iteration off, and with its check failing at chosen iterations; and on the degenerate free sets.

osfm_ba_report does not say which path an iteration took.  That the default runs take the straight-line iteration rests on the condition
the solver itself uses (SolvePlan::exact_expected: exact band, exact border or constant cameras, no trace); the tests assert the part of
it the report shows, preconditioner_bandwidth == shot_bandwidth."""
import numpy as np
import pytest

import ba_recovery_cases as rc

pytestmark = pytest.mark.gpu

KNOBS = ("OSFM_BA_NO_FAST", "OSFM_BA_FAST_FAIL_AT", "OSFM_BA_NO_SBAND", "OSFM_BA_WIDE_LDLT", "OSFM_BA_TRACE", "OSFM_BA_BAND_PER_SHOT", "OSFM_BA_CHECK_BAND")
BA_KEYS = ("cost_history", "shot_pose", "points", "cam_params")


def _solve(monkeypatch, name, env=None, problem=None, general=None, **overrides):
    """one solve of a scene with exactly the switches of `env` set (the solver reads them at every call)"""
    from opensfm_amd import bundle

    general = rc.solver(name) == "general" if general is None else general
    with monkeypatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        fn = bundle.bundle_general_arrays if general else bundle.bundle_arrays
        return fn(rc.problem(name) if problem is None else problem, rc.config(name), **rc.NO_TOL, **overrides)


def _as_general(pr):
    import test_oracle_bundle_general as og

    return og._as_general(pr)


# ---- rejected steps against the oracle ----------------------------------------------------------------------------------------------
# (scene, switches, options, exact band expected, through osfm_bundle_solve)
REJECTION_RUNS = {
    "narrow20-one_workgroup_band": ("narrow20", {}, {}, True, False),
    "narrow20-cyclic_reduction_in_lds": ("narrow20", {"OSFM_BA_NO_SBAND": "1"}, {}, True, False),
    "narrow20-block_jacobi": ("narrow20", {}, {"preconditioner": 1}, False, False),  # careful path, many CG iterations per step
    "narrow20-generic_rows": ("narrow20", {}, {}, True, True),  # the generic rows of a [k1 k2 focal] problem
    "wide40-dense_clusters": ("wide40", {}, {}, True, False),
    "wide40-block_ldlt": ("wide40", {"OSFM_BA_WIDE_LDLT": "1"}, {}, True, False),
    "grid6x14-dense_clusters": ("grid6x14", {}, {}, True, False),
    "local30": ("local30", {}, {}, True, False),
    "s1025": ("s1025", {}, {}, True, False),
    "gen_spherical": ("gen_spherical", {}, {}, True, False),
    "gen_brown": ("gen_brown", {}, {}, True, False),
}


@pytest.mark.parametrize("run", sorted(REJECTION_RUNS))
def test_rejected_steps_match_oracle(oracle_lib, gpu_ctx, monkeypatch, run):
    """the oracle's trajectory with its rejections (rc.check_against_oracle: counts, the rejected iterations, cost history to 1e-7, RMSE to
    1e-4 px), whichever factorisation carries the band"""
    name, env, options, exact, as_general = REJECTION_RUNS[run]
    o = rc.oracle_solve(oracle_lib, name)
    assert rc.rejected(o["cost_history"]) == rc.recorded(name)  # (the premise, kept by tests/test_ba_recovery_premises.py)
    if as_general:
        g = _solve(monkeypatch, name, env, problem=_as_general(rc.problem(name)), general=True, **options)
    else:
        g = _solve(monkeypatch, name, env, **options)
    rc.check_against_oracle(g, o)
    if exact:  # the premise of the straight-line iteration, as far as the report shows it: the preconditioner is the exact band
        assert g["preconditioner_bandwidth"] == g["shot_bandwidth"] >= 1, (g["preconditioner_bandwidth"], g["shot_bandwidth"])
    else:
        assert g["preconditioner_bandwidth"] == 0 and g["pcg_iterations"] > 3 * g["iterations"]
    if name in ("wide40", "grid6x14"):
        assert g["shot_bandwidth"] > 10  # beyond the clusters in LDS: the wide band
    if name == "s1025":
        assert len(rc.problem(name)["shot_pose"]) == 1025


# ---- the straight-line iteration and its way back -----------------------------------------------------------------------------------
def _fail_at(name):
    """LM iterations at which the straight-line check is made to fail: the first, the first rejected one, the one behind every run of
    rejections, the last"""
    rej = rc.recorded(name)
    ks = {1, rej[0], rc.config(name)["bundle_max_iterations"]}
    for i, r in enumerate(rej):
        if i > 0 and rej[i - 1] == r - 1 and r + 1 not in rej:
            ks.add(r + 1)
    assert rc.first_run_of_rejections(rej)[1] + 1 in ks
    return sorted(ks)


def _path_runs(monkeypatch, name):
    """label -> solve: the default (straight-line iterations), the careful path alone, and a failed check at each iteration of _fail_at"""
    runs = {"default": _solve(monkeypatch, name), "careful": _solve(monkeypatch, name, {"OSFM_BA_NO_FAST": "1"})}
    for k in _fail_at(name):
        runs["fail_at_%d" % k] = _solve(monkeypatch, name, {"OSFM_BA_FAST_FAIL_AT": str(k)})
    return runs


@pytest.mark.parametrize("name", ["narrow20", "local30", "wide40", "s1025"])
def test_straight_line_iteration_and_its_way_back_are_the_careful_path_bit_for_bit(oracle_lib, gpu_ctx, monkeypatch, name):
    """[k1 k2 focal] kernels: every reduction has a fixed order, so the straight-line iteration, the careful path, and an iteration redone on
    the careful path after a failed check -- at the first iteration, at a rejected one, right behind a run of rejections, at the last --
    give the same bits (the claim above relinearise_old_point, and what tests/test_emu_ba.py asserts on the host emulation)"""
    runs = _path_runs(monkeypatch, name)
    careful = runs["careful"]
    rc.check_against_oracle(careful, rc.oracle_solve(oracle_lib, name))
    assert careful["preconditioner_bandwidth"] == careful["shot_bandwidth"]
    different = []
    for label, g in runs.items():
        for k in BA_KEYS:
            if not np.array_equal(g[k], careful[k]):
                different.append((label, k, float(np.max(np.abs(g[k] - careful[k]))) if g[k].shape == careful[k].shape else None))
        if (g["iterations"], g["successful_steps"]) != (careful["iterations"], careful["successful_steps"]):
            different.append((label, "iterations / successful_steps", (g["iterations"], g["successful_steps"])))
    print("%s: runs %s; rejected on the device %s; different from the careful run: %s" % (name, sorted(runs), rc.rejected(careful["cost_history"]), different))
    assert not different, different
    # Other first-iterate tolerances; each pair of runs is compared with each other only.
    #   0: no first iterate is accepted as a direct solve.  (SolvePlan::exact_expected asks for pcg_direct_tolerance > pcg_tolerance, so
    #      the straight-line iteration is not tried at all: both runs walk the careful path.)
    #   just above pcg_tolerance: the straight-line iteration IS tried, and its check fails by itself -- not by the knob -- at the first LM
    #      iteration whose direct solve leaves a relative residual above 1e-10.  That this happens is read off the careful run: it needed
    #      a second CG iteration somewhere (narrow20 and wide40; local30 and s1025 stay below 1e-10 throughout, their pair rides along).
    for tol in (0.0, 1.0000001e-10):
        a = _solve(monkeypatch, name, pcg_direct_tolerance=tol)
        b = _solve(monkeypatch, name, {"OSFM_BA_NO_FAST": "1"}, pcg_direct_tolerance=tol)
        print("%s: pcg_direct_tolerance %g: %d / %d CG iterations in %d LM iterations" % (name, tol, a["pcg_iterations"], b["pcg_iterations"], b["iterations"]))
        for k in BA_KEYS:
            assert np.array_equal(a[k], b[k]), (tol, k)
        assert (a["iterations"], a["successful_steps"], a["pcg_iterations"]) == (b["iterations"], b["successful_steps"], b["pcg_iterations"])
        if tol > 0 and name in ("narrow20", "wide40"):
            assert b["pcg_iterations"] > b["iterations"]  # the premise: some first iterate missed the tolerance


@pytest.mark.parametrize("name", ["gen_spherical", "gen_brown"])
def test_generic_mode_paths_each_match_oracle(oracle_lib, gpu_ctx, monkeypatch, name):
    """generic rows: the prior blocks and gradients are summed with floating-point atomics, so the runs are not claimed equal in bits; each
    of them -- default, careful, a failed check at every iteration of _fail_at, pcg_direct_tolerance = 0 with and without the straight-line
    iteration -- is held to the oracle, and to nothing measured on the code under test.  After a failed check the factorisation and the
    right-hand side of one accumulation meet rows and gradients of another (relinearise_old_point): if that pairing mattered it would show
    here, in the iteration that is redone and in the steps after it."""
    o = rc.oracle_solve(oracle_lib, name)
    runs = _path_runs(monkeypatch, name)
    runs["direct_tolerance_0"] = _solve(monkeypatch, name, pcg_direct_tolerance=0.0)
    runs["direct_tolerance_0_careful"] = _solve(monkeypatch, name, {"OSFM_BA_NO_FAST": "1"}, pcg_direct_tolerance=0.0)
    worst = {label: rc.max_rel_cost_diff(g, o) for label, g in runs.items()}
    bits = {label: bool(np.array_equal(g["cost_history"], runs["careful"]["cost_history"])) for label, g in runs.items()}
    print("%s: largest relative cost-history difference from the oracle per run %s; cost history bit-equal to the careful run %s" % (name, worst, bits))
    for label, g in runs.items():
        rc.check_against_oracle(g, o)
        assert g["preconditioner_bandwidth"] == g["shot_bandwidth"], label


# ---- degenerate free sets --------------------------------------------------------------------------------------------------------------
def _solve_problem(monkeypatch, pr, general, iters, **overrides):
    from opensfm_amd import bundle

    with monkeypatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        fn = bundle.bundle_general_arrays if general else bundle.bundle_arrays
        return fn(pr, {"bundle_max_iterations": iters}, **overrides)


def _ordinary(oracle_lib, monkeypatch):
    pr = rc.degenerate_base()
    if "ordinary" not in rc._ORACLE:
        rc._ORACLE["ordinary"] = oracle_lib.ba_solve(pr, max_iterations=4, **rc.NO_TOL)
    o = rc._ORACLE["ordinary"]
    g = _solve_problem(monkeypatch, pr, False, 4, **rc.NO_TOL)
    assert g["iterations"] == o["iterations"] == 4 and g["successful_steps"] == o["successful_steps"]
    assert np.allclose(g["cost_history"], o["cost_history"], rtol=1e-7, atol=0)


@pytest.mark.parametrize("general", [False, True], ids=["k1k2focal", "generic_rows"])
@pytest.mark.parametrize("name", sorted(rc.DEGENERATE_SETS))
def test_degenerate_free_sets_match_oracle(oracle_lib, gpu_ctx, monkeypatch, name, general):
    """an empty reduced system (points only), the border alone (camera only), shots only, one free shot among constant ones, one free point,
    nothing free at all: the oracle's iterations, termination and costs; constant blocks come back bit for bit; and the context still solves
    an ordinary problem afterwards"""
    flat = rc.degenerate_problem(name)
    pr = rc.degenerate_problem(name, general=True) if general else flat
    # each solver against its own oracle: the two differ in the cost of a constant shot's position prior (Ceres folds residual blocks over
    # constant parameter blocks into the cost: oracle.bundle_general and osfm_bundle_solve count it, the [k1 k2 focal] pair leaves it out)
    if general:
        o = oracle_lib.bundle_general(pr, max_iterations=rc.DEGENERATE_ITERATIONS, **rc.NO_TOL)
    else:
        o = oracle_lib.ba_solve(pr, max_iterations=rc.DEGENERATE_ITERATIONS, **rc.NO_TOL)
    g = _solve_problem(monkeypatch, pr, general, rc.DEGENERATE_ITERATIONS, **rc.NO_TOL)
    poses, cams = (g["rig_instance_pose"], g["cam_params"][:, :3]) if general else (g["shot_pose"], g["cam_params"])
    print("%s: iterations %d / %d, termination %d / %d, successful %d / %d, largest relative cost difference %.3e"
          % (name, g["iterations"], o["iterations"], g["termination"], o["termination"], g["successful_steps"], o["successful_steps"], rc.max_rel_cost_diff(g, o)))
    assert g["iterations"] == o["iterations"] and g["termination"] == o["termination"] and g["successful_steps"] == o["successful_steps"]
    assert np.allclose(g["cost_history"], o["cost_history"], rtol=1e-7, atol=0), (g["cost_history"], o["cost_history"])
    if name == "nothing":
        assert g["iterations"] == 0 and g["termination"] == 2
    else:
        assert g["iterations"] == rc.DEGENERATE_ITERATIONS and g["successful_steps"] > 0  # something was free, and it moved
    for got, given, fixed in ((poses, flat["shot_pose"], flat["shot_fixed"]), (g["points"], flat["points"], flat["point_fixed"]),
                              (cams, flat["cam_params"], flat["cam_fixed"])):
        assert np.array_equal(got[fixed == 1], np.asarray(given, float)[fixed == 1])
        if (fixed == 0).any():
            assert np.abs(got[fixed == 0] - np.asarray(given, float)[fixed == 0]).max() > 0
    _ordinary(oracle_lib, monkeypatch)


@pytest.mark.parametrize("general", [False, True], ids=["k1k2focal", "generic_rows"])
def test_gradient_tolerance_stops_before_the_first_iteration(oracle_lib, gpu_ctx, monkeypatch, general):
    """termination 2 (the one value no other GPU test asserts): max |gradient| of the first point is below a tolerance of 1e9, the loop
    ends before its first iteration and the inputs come back bit for bit"""
    pr = rc.degenerate_base()
    tol = dict(function_tolerance=0.0, gradient_tolerance=1e9, parameter_tolerance=0.0)
    if general:
        o = oracle_lib.bundle_general(_as_general(pr), max_iterations=rc.DEGENERATE_ITERATIONS, **tol)
    else:
        o = oracle_lib.ba_solve(pr, max_iterations=rc.DEGENERATE_ITERATIONS, **tol)
    g = _solve_problem(monkeypatch, _as_general(pr) if general else pr, general, rc.DEGENERATE_ITERATIONS, **tol)
    assert o["termination"] == 2 and o["iterations"] == 0
    assert g["termination"] == 2 and g["iterations"] == 0 and g["successful_steps"] == 0
    assert g["initial_cost"] == pytest.approx(o["initial_cost"], rel=1e-12) and g["final_cost"] == g["initial_cost"]
    poses, cams = (g["rig_instance_pose"], g["cam_params"][:, :3]) if general else (g["shot_pose"], g["cam_params"])
    assert np.array_equal(poses, pr["shot_pose"]) and np.array_equal(g["points"], pr["points"]) and np.array_equal(cams, pr["cam_params"])
    _ordinary(oracle_lib, monkeypatch)
