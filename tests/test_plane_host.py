"""The plane-based two-view solve (opensfm_amd/csrc/plane_core.h), compiled for the host with loops in place of lanes
(tests/native/plane_host.cpp), against the numpy restatement of tests/plane_cases.py: the normalised DLT and the decomposition against
the restatement with bounds taken from the restatement's own distance to a 50-digit evaluation, the eight motions against the
reference's own motion_from_plane_homography as a set, the choice over a table of counts, whole pairs (planted inlier sets, the chosen
motion, its inlier list), a batch against its single calls, and a stand-alone program under the address and undefined-behaviour
sanitizers."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import plane_cases as cases

# The restatement's own largest distance from the 50-digit DLT over leaf_dlt_cases() (H scaled to Frobenius norm 1, equal sign) is
# 1.301e-09, on "mixed-4": three neighbouring points and a far one, the worst conditioned of the 4-point sets (the well spread set shows
# 1.4e-14, sets of 12 rows and more 1e-15).  Both sides solve the normal equations, so both carry the square of the condition number;
# the host build is allowed 100 times the restatement's own error.  (Measured for the host build: 1.103e-09 from the restatement and
# 1.976e-10 from the 50-digit H on that case.)
RESTATEMENT_DLT_ERROR = 1.301e-09
DLT_BOUND = 100 * RESTATEMENT_DLT_ERROR
# The same for the decomposition over leaf_homographies(): the restatement's largest distance from the 50-digit motions is 1.776e-14 over
# all 8 x 16 numbers (the host build's own: 1.704e-14); the bound is 100 times that.
RESTATEMENT_MOTIONS_ERROR = 1.776e-14
MOTIONS_BOUND = 100 * RESTATEMENT_MOTIONS_ERROR
# the largest |aa_to_rotmat(rotation) - R| entry of a chosen rotation: one unit in the last place of an entry near 1 is 2.22e-16; 100 times
AA_ROUND_TRIP_BOUND = 2.22e-14

REF = "/root/reference/opensfm"


@pytest.fixture(scope="module")
def host():
    return cases.build_host()


@pytest.fixture(scope="module")
def all_cases():
    return cases.cases()


@pytest.fixture(scope="module")
def hosted(host, all_cases):
    """the mixed batch in one call: [(HostResult, mask of the pair)]"""
    b1, b2, off = cases.batch(all_cases)
    res, mask = cases.host_pairs(host, b1, b2, off)
    return [(res[k], mask[off[k]: off[k + 1]]) for k in range(len(all_cases))]


def test_dlt_matches_the_restatement_within_its_own_error(host):
    worst_restated, worst_host = 0.0, 0.0
    for name, x1, x2, idx in cases.leaf_dlt_cases():
        truth = cases.unit_frobenius(cases.mp_dlt(x1[idx], x2[idx]))
        restated = cases.unit_frobenius(cases.dlt(x1[idx], x2[idx]), truth)
        for wave in (False, True):  # the sequential sum order and the final fit's
            H = cases.host_dlt(host, x1, x2, idx, wave=wave)
            assert H is not None and np.linalg.det(H) > 0, name
            got = cases.unit_frobenius(H, truth)
            print("%s (wave %d): restatement - truth %.3e, host - truth %.3e, host - restatement %.3e"
                  % (name, wave, np.abs(restated - truth).max(), np.abs(got - truth).max(), np.abs(got - restated).max()))
            worst_host = max(worst_host, np.abs(got - restated).max())
        worst_restated = max(worst_restated, np.abs(restated - truth).max())
    assert worst_restated <= 10 * RESTATEMENT_DLT_ERROR, worst_restated  # the constant above is the value measured; LAPACK builds differ a little
    assert worst_host <= DLT_BOUND, worst_host


def test_dlt_has_no_model_for_rows_behind_a_camera_or_coincident_points(host):
    nan = float("nan")
    x = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    assert cases.host_dlt(host, x, x, np.arange(4)) is not None
    bad = x.copy()
    bad[2] = nan
    assert cases.host_dlt(host, bad, x, np.arange(4)) is None and cases.host_dlt(host, x, bad, np.arange(4), wave=True) is None
    same = np.tile([[0.25, -0.5]], (4, 1))
    assert cases.host_dlt(host, same, x, np.arange(4)) is None  # the scale of side 1 is not finite
    assert cases.host_dlt(host, x, x, np.arange(3)) is None  # fewer than 4 rows


def test_motions_match_the_restatement_in_order(host):
    worst_restated, worst_host = 0.0, 0.0
    for name, H, (R_true, t_true) in cases.leaf_homographies():
        got, singular = cases.host_motions(host, H)
        want = cases.flat_motions(cases.motions(H))
        truth = cases.mp_motions(H)
        print("%s: restatement - truth %.3e, host - truth %.3e, host - restatement %.3e"
              % (name, np.abs(want - truth).max(), np.abs(got - truth).max(), np.abs(got - want).max()))
        worst_restated = max(worst_restated, np.abs(want - truth).max())
        worst_host = max(worst_host, np.abs(got - want).max())
        assert abs(singular[1] - 1.0) <= 1e-14 and singular[0] > singular[1] > singular[2] > 0, name
        for m in got:
            R = m[:9].reshape(3, 3)
            assert np.abs(R.dot(R.T) - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14, name
        assert min(max(np.abs(m[:9].reshape(3, 3) - R_true).max(), np.abs(m[9:12] - t_true).max()) for m in got) <= MOTIONS_BOUND, name
    assert worst_restated <= 10 * RESTATEMENT_MOTIONS_ERROR, worst_restated  # the constant above is the value measured; LAPACK builds differ a little
    assert worst_host <= MOTIONS_BOUND, worst_host


def test_motions_reject_nearly_equal_singular_values(host):
    got, _ = cases.host_motions(host, cases.rodrigues([0.1, -0.2, 0.05]))  # a rotation: all three equal
    assert got is None and cases.motions(cases.rodrigues([0.1, -0.2, 0.05])) is None
    H = np.diag([1.00005, 1.0, 0.9])  # d1 / d2 below 1.0001
    assert cases.host_motions(host, H)[0] is None and cases.motions(H) is None
    H = np.diag([1.2, 1.0, 0.99995])  # d2 / d3 below 1.0001
    assert cases.host_motions(host, H)[0] is None and cases.motions(H) is None
    assert cases.host_motions(host, np.diag([1.2, 1.0, 0.9]))[0] is not None


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference is not mounted")
def test_motions_equal_the_reference_s_own_as_a_set(host):
    """multiview.motion_from_plane_homography loaded from the reference's file (stand-ins for what it imports): the same eight motions;
    its order follows LAPACK's signs, so they are matched as a set"""

    class Stub(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            cls = type(name, (), {})
            setattr(self, name, cls)
            return cls

    names = ["cv2", "opensfm", "opensfm.pygeometry", "opensfm.pymap", "opensfm.pyrobust", "opensfm.transformations", "opensfm.multiview"]
    saved = {k: sys.modules.get(k) for k in names}
    try:
        pkg = Stub("opensfm")
        pkg.__path__ = [REF]
        sys.modules["cv2"] = Stub("cv2")
        sys.modules["opensfm"] = pkg
        for name in ("pygeometry", "pymap", "pyrobust"):
            sys.modules["opensfm." + name] = Stub("opensfm." + name)
            setattr(pkg, name, sys.modules["opensfm." + name])
        for name in ("transformations", "multiview"):
            spec = importlib.util.spec_from_file_location("opensfm." + name, os.path.join(REF, name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules["opensfm." + name] = mod
            setattr(pkg, name, mod)
            spec.loader.exec_module(mod)
        multiview = sys.modules["opensfm.multiview"]
        for name, H, _ in cases.leaf_homographies():
            got, _ = cases.host_motions(host, H)
            ref = cases.flat_motions(multiview.motion_from_plane_homography(H))
            assert len(ref) == 8
            used = set()
            for m in got:
                k = int(np.argmin([np.abs(m - r).max() for r in ref]))
                assert np.abs(m - ref[k]).max() <= MOTIONS_BOUND, (name, np.abs(m - ref[k]).max())
                used.add(k)
            assert len(used) == 8, name
        assert multiview.motion_from_plane_homography(cases.rodrigues([0.1, -0.2, 0.05])) is None
    finally:
        for k in names:
            sys.modules.pop(k, None)
        sys.modules.update({k: v for k, v in saved.items() if v is not None})


def test_pick_takes_the_most_inliers_and_the_lowest_index_on_ties(host):
    table = [([0] * 8, 0), ([1, 3, 2, 0, 0, 0, 0, 0], 1), ([5, 0, 5, 0, 0, 0, 0, 0], 0), ([0, 0, 0, 0, 0, 0, 0, 9], 7), ([2, 7, 7, 7, 1, 7, 0, 7], 1),
             ([0, 0, 4, 0, 4, 0, 3, 0], 2), ([9, 9, 9, 9, 9, 9, 9, 9], 0), ([0, 1, 2, 3, 4, 5, 6, 7], 7), ([7, 6, 5, 4, 3, 2, 1, 0], 0)]
    for counts, want in table:
        arr = (C.c_int * 8)(*counts)
        assert host.host_plane_pick(arr) == want == int(np.argmax(counts)), counts


def test_whole_pairs(host, all_cases, hosted):
    seen, compared = set(), 0
    for c, (got, mask) in zip(all_cases, hosted):
        n = len(c.b1)
        all_behind = bool((c.b2[:, 2] <= 0).all())
        assert len(mask) == n
        if got.status != cases.OK:
            assert got.chosen == -1 and got.n_inliers == 0 and not any(got.motion_inliers) and not (mask >> 1).any(), c.name
            assert not any(got.R) and not any(got.t) and not any(got.rotation) and not any(got.translation), c.name
            if got.status == cases.NO_HOMOGRAPHY:
                assert got.h_inliers == 0 and not mask.any() and not any(got.H) and not any(got.singular), c.name
            else:
                assert np.array_equal(np.flatnonzero(mask & 1), c.planted) and got.h_inliers == len(c.planted), c.name
                s = np.array(got.singular)
                assert s[0] / s[1] < 1.0001 or s[1] / s[2] < 1.0001, c.name
            seen.add(cases.outcome(n, got.status, None, all_behind))
            compared += 1
            continue
        # the planted inlier set is the only one a correct RANSAC can return
        assert np.array_equal(np.flatnonzero(mask & 1), c.planted) and got.h_inliers == len(c.planted), c.name
        H = np.array(got.H).reshape(3, 3)
        s = np.linalg.svd(H)[1]
        assert abs(s[1] - 1.0) <= 1e-14 and np.linalg.det(H) > 0 and np.abs(s - np.array(got.singular)).max() <= 1e-14, c.name
        ms = cases.motions(H)
        lists = [cases.motion_inliers(c.b1, c.b2, R, t, cases.THRESHOLD) for R, t, _, _ in ms]
        counts = [len(x) for x in lists]
        assert list(got.motion_inliers) == counts, c.name
        chosen = int(np.argmax(counts))  # the first among the maximal ones
        assert got.chosen == chosen and got.n_inliers == counts[chosen], c.name
        assert np.array_equal(np.flatnonzero(mask >> 1 & 1), lists[chosen]), c.name
        assert np.abs(np.array(got.R).reshape(3, 3) - ms[chosen][0]).max() <= MOTIONS_BOUND, c.name
        assert np.abs(np.array(got.t) - ms[chosen][1]).max() <= MOTIONS_BOUND and list(got.translation) == list(got.t), c.name
        # the true motion is among the maximal ones; it explains every planted row and, where there are any, the off-plane rows
        R_true, t_true = c.truth
        err = [max(np.abs(R - R_true).max(), np.abs(t - t_true).max()) for R, t, _, _ in ms]
        k_true = int(np.argmin(err))
        assert err[k_true] < 2e-3 and counts[k_true] == max(counts) and set(c.planted) <= set(lists[k_true]), (c.name, err[k_true])
        if c.expect == "winner":
            assert chosen == k_true and counts[k_true] > len(c.planted), c.name
        aa, R = np.array(got.rotation), np.zeros(9)
        host.host_plane_aa_to_rotmat(aa.ctypes.data_as(cases.DP), R.ctypes.data_as(cases.DP))
        assert np.abs(R - np.array(got.R)).max() <= AA_ROUND_TRIP_BOUND, c.name
        o = cases.outcome(n, got.status, counts, all_behind)
        if c.expect is not None:
            assert o == c.expect, (c.name, o, counts)
        seen.add(o)
        compared += 1
    assert compared == len(all_cases)  # no pair is skipped
    assert seen == cases.OUTCOMES, seen


def test_a_batch_equals_its_single_calls_byte_for_byte(host, all_cases, hosted):
    for c, (got, mask) in zip(all_cases, hosted):
        res, m = cases.host_pairs(host, c.b1, c.b2, [0, len(c.b1)])
        assert cases.result_bytes(res[0]) == cases.result_bytes(got), c.name
        assert m.tobytes() == mask.tobytes(), c.name


def test_standalone_program_under_sanitizers():
    exe = cases.compile_native("plane_main", os.path.join(cases.NATIVE, "plane_main.cpp"),
                               ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], shared=False)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "plane_main: ok" in done.stdout
