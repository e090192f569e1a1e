"""The two-view 5-point finish (opensfm_amd/csrc/twoview_core.h), compiled for the host with loops in place of lanes
(tests/native/twoview_host.cpp), against the restatement of tests/twoview_cases.py composed from the CPU oracle's leaves: statuses,
chosen configurations, both inlier lists and R / t of both configurations bit for bit; the angle-axis of the chosen rotation; the
decision rule over a table of counts; and a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import twoview_cases as cases

# the largest |aa_to_rotmat(rotation) - R| entry the host build shows over the 38 chosen rotations of this file's cases is 2.220e-16 (one
# unit in the last place of an entry near 1); the bound is 100 times that
AA_ROUND_TRIP_BOUND = 2.22e-14


@pytest.fixture(scope="module")
def host():
    return cases.build_host()


@pytest.fixture(scope="module")
def all_cases():
    return cases.ransac_cases() + cases.given_pose_cases()


@pytest.fixture(scope="module")
def restated(all_cases):
    return [cases.restate(c) for c in all_cases]


@pytest.fixture(scope="module")
def hosted(host, all_cases):
    """the host build over the same cases, one call per (mode, parameter set): [(HostResult, mask of the pair)] in case order"""
    out = [None] * len(all_cases)
    index = {id(c): k for k, c in enumerate(all_cases)}
    for given in (False, True):
        for (threshold, check_reversal, ratio), group in cases.by_params([c for c in all_cases if (c.pose is not None) == given]).items():
            b1, b2, off, poses = cases.batch(group)
            res, mask = cases.host_pairs(host, b1, b2, off, poses, threshold, check_reversal, ratio)
            for k, c in enumerate(group):
                out[index[id(c)]] = (res[k], mask[off[k]: off[k + 1]])
    return out


def _counts(r):
    return [len(c[2]) for c in r["configs"]] + [-1] * (2 - len(r["configs"]))


def test_restatement_reaches_every_outcome(all_cases, restated):
    seen = set()
    for c, r in zip(all_cases, restated):
        n0, n1 = _counts(r)
        seen.add(cases.outcome(r["status"], r["chosen"], n0, n1))
        if c.expect is not None:
            assert (r["status"], r["chosen"]) == c.expect, (c.name, r["status"], r["chosen"], n0, n1)
    assert seen == cases.OUTCOMES, seen
    assert len(restated) == len(all_cases)


def test_host_build_matches_the_restatement_bit_for_bit(all_cases, restated, hosted):
    compared = 0
    for c, want, (got, mask) in zip(all_cases, restated, hosted):
        assert (got.status, got.chosen) == (want["status"], want["chosen"]), c.name
        assert len(mask) == len(c.b1)
        if len(c.b1) <= 5:
            assert list(got.n_inliers) == [-1, -1] and not mask.any(), c.name
            compared += 1
            continue
        for k, (R, t, inliers, its) in enumerate(want["configs"]):
            assert np.array_equal(np.flatnonzero(mask >> k & 1), inliers), (c.name, k)
            assert got.n_inliers[k] == len(inliers) and got.refine_iterations[k] == its, (c.name, k)
            assert np.array(got.R[9 * k: 9 * k + 9]).tobytes() == np.ascontiguousarray(R).tobytes(), (c.name, k)
            assert np.array(got.t[3 * k: 3 * k + 3]).tobytes() == np.ascontiguousarray(t).tobytes(), (c.name, k)
        if not c.check_reversal:
            assert got.n_inliers[1] == -1 and not (mask >> 1 & 1).any(), c.name
        chosen = want["configs"][want["chosen"]][2] if want["chosen"] >= 0 else []
        assert np.array_equal(np.flatnonzero(mask >> 2 & 1), chosen), c.name
        if want.get("ransac"):
            r = want["ransac"]
            assert (got.score, got.iterations) == (r["score"], r["iterations"]), c.name
            assert np.array(got.lo_model).tobytes() == np.ascontiguousarray(r["lo_model"]).tobytes(), c.name
        compared += 1
    assert compared == len(all_cases)  # no pair is skipped


def test_angle_axis_reproduces_the_chosen_rotation(host, all_cases, hosted):
    worst, checked = 0.0, 0
    for c, (got, _) in zip(all_cases, hosted):
        if got.status != cases.OK:
            assert not any(got.rotation) and not any(got.translation), c.name
            continue
        aa, R = np.array(got.rotation), np.zeros(9)
        host.host_aa_to_rotmat(aa.ctypes.data_as(C.POINTER(C.c_double)), R.ctypes.data_as(C.POINTER(C.c_double)))
        worst = max(worst, float(np.abs(R - np.array(got.R[9 * got.chosen: 9 * got.chosen + 9])).max()))
        assert list(got.translation) == list(got.t[3 * got.chosen: 3 * got.chosen + 3]), c.name
        checked += 1
    print("largest |aa_to_rotmat(rotation) - R| over %d chosen rotations: %.3e" % (checked, worst))
    assert checked > 20 and worst <= AA_ROUND_TRIP_BOUND, worst


def test_decision_rule_over_a_table_of_counts(host):
    for check_reversal in (0, 1):
        for ratio in (0.5, 0.95, 1.0):
            for n0 in (-1, 0, 5, 6, 7, 19, 20, 100):
                for n1 in (-1, 0, 5, 6, 7, 19, 20, 100):
                    chosen = C.c_int(-7)
                    status = host.host_two_view_decide(n0, n1, check_reversal, ratio, C.byref(chosen))
                    assert (status, chosen.value) == cases.decide(n0, n1, bool(check_reversal), ratio), (n0, n1, check_reversal, ratio)
    chosen = C.c_int(-7)
    assert host.host_two_view_decide(20, 20, 1, 1.0, C.byref(chosen)) == cases.OK and chosen.value == 1  # a tie picks the transposed one
    assert host.host_two_view_decide(19, 20, 1, 0.95, C.byref(chosen)) == cases.OK and chosen.value == 1  # 0.95 is not above 0.95
    assert host.host_two_view_decide(96, 100, 1, 0.95, C.byref(chosen)) == cases.UNDECIDABLE and chosen.value == -1


def test_refinement_alone_matches_the_oracle_bit_for_bit(host):
    """skip_inlier_tests: configuration 0 on a given pose is relative_pose_refinement over all correspondences"""
    import oracle

    b1, b2, R, t = cases.scene(np.random.default_rng(7), 101, outliers=0.0)
    noisy = cases.rodrigues(np.array([0.01, -0.02, 0.015])) @ R
    pose = (cases.transposed3(noisy), cases.inverse_translation(noisy, t))
    res, mask = cases.host_pairs(host, b1, b2, [0, 101], np.r_[pose[0].reshape(9), pose[1]].reshape(1, 12), cases.THRESHOLD, False, 1.0,
                                 refine_iterations=20, skip_inlier_tests=True)
    start = np.c_[cases.transposed3(pose[0]), cases.inverse_translation(pose[0], pose[1])]
    refined, its, _ = oracle.relative_pose_refinement(start, b1, b2, 20)
    assert res[0].n_inliers[0] == 101 and (mask & 1).all() and res[0].refine_iterations[0] == its and its > 1
    assert np.array(res[0].R[:9]).tobytes() == np.ascontiguousarray(refined[:, :3]).tobytes()
    Rc = cases.transposed3(refined[:, :3])
    assert np.array(res[0].t[:3]).tobytes() == cases.inverse_translation(Rc, cases.inverse_translation(refined[:, :3], refined[:, 3])).tobytes()


def test_standalone_program_under_sanitizers():
    exe = cases.compile_native("twoview_main", os.path.join(cases.NATIVE, "twoview_main.cpp"),
                               ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], shared=False)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "twoview_main: ok" in done.stdout
