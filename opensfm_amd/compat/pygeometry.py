"""Leaves of the reference's ``pygeometry`` (``opensfm/src/geometry/python/pybind.cc``) under its argument names:
``triangulate_bearings_midpoint`` and ``point_refinement``, served by ``triangulate.hip``, and ``absolute_pose_three_points`` and
``absolute_pose_n_points``, served by ``abspose.hip``, and ``relative_pose_refinement``, served by ``twoview.hip``.  One call is one
track (or pair) on the GPU -- these exist so that
code written against the leaves (``TrackTriangulator``) runs unchanged; the batched path is
``opensfm_amd.reconstruction.triangulate_shot_features`` / ``retriangulate``.

This module is NOT registered by ``compat.install()`` (``compat.MODULES`` stays as it is): import it directly,
``from opensfm_amd.compat import pygeometry``."""
from typing import List, Sequence, Tuple

import numpy as np

from .. import reconstruction as _reconstruction
from .._lib import check as _check, default_context as _default_context, load as _load


def triangulate_bearings_midpoint(centers, bearings, threshold_list: Sequence[float], min_angle: float, min_depth: float) -> Tuple[bool, np.ndarray]:
    """``geometry::TriangulateBearingsMidpoint`` (triangulation.cc:139-178): (valid, X).  ``min_angle`` in radians.  A threshold list
    shorter than the rows returns (False, ...) as the reference does; the device call takes ONE threshold, so thresholds that are not all
    equal raise NotImplementedError.  X is NaN when the triangulation is not valid (the reference returns an uninitialised vector), and a
    midpoint that is not finite is not valid (the one divergence of ``osfm_triangulate_bearings``)."""
    centers = np.ascontiguousarray(centers, np.float64).reshape(-1, 3)
    bearings = np.ascontiguousarray(bearings, np.float64).reshape(-1, 3)
    thresholds = np.asarray(threshold_list, np.float64).reshape(-1)
    if len(thresholds) < len(centers):
        return False, np.full(3, np.nan)
    thresholds = thresholds[: len(centers)]
    if len(thresholds) and not (thresholds == thresholds[0]).all():
        raise NotImplementedError("triangulate_bearings_midpoint: one threshold per call on the GPU path; the list holds different values")
    if len(centers) < 2:  # (the pair loop of the reference finds no pair)
        return False, np.full(3, np.nan)
    # refinement_iterations = 0: the solver evaluates once and takes no step, so the point that comes back is the midpoint
    points, status, _, _ = _reconstruction.triangulate_bearings_arrays(centers, bearings, [0, len(centers)], float(thresholds[0]),
                                                                     float(np.degrees(min_angle)), float(min_depth), 0)
    return bool(status[0] == 0), points[0].copy()


def point_refinement(centers, bearings, point, iterations: int) -> np.ndarray:
    """``geometry::PointRefinement`` (triangulation.cc:221-233): TinySolver with ``max_num_iterations = iterations`` from ``point``"""
    import ctypes as C

    centers = np.ascontiguousarray(centers, np.float64).reshape(-1, 3)
    bearings = np.ascontiguousarray(bearings, np.float64).reshape(-1, 3)
    if len(centers) != len(bearings):
        raise ValueError("point_refinement: centers and bearings do not agree")
    initial = np.ascontiguousarray(point, np.float64).reshape(3)
    offsets = np.array([0, len(centers)], np.int64)
    out, used, ms = np.full(3, np.nan), np.zeros(1, np.int32), C.c_double(0.0)

    def ptr(a, t):
        return a.ctypes.data_as(C.POINTER(t))

    _check(_load().osfm_triangulate_refine(_default_context().handle, ptr(centers, C.c_double), ptr(bearings, C.c_double), ptr(offsets, C.c_int64), 1,
                                           ptr(initial, C.c_double), int(iterations), ptr(out, C.c_double), ptr(used, C.c_int32), C.byref(ms)),
           "osfm_triangulate_refine")
    return out


def relative_pose_refinement(Rt, b1, b2, iterations: int) -> np.ndarray:
    """``geometry::RelativePoseRefinement`` (relative_pose.h:149-183): the 3 x 4 pose [R | t] refined by TinySolver over 100 rand()-picked
    correspondences, ``multiview.relative_pose_optimize_nonlinear`` runs unchanged on it.  Served by ``twoview.hip``: one pair, the
    given pose, every correspondence counted as an inlier.  The device call takes and returns the inverse pose, so Rt is inverted going
    in and coming out (two roundings of the translation, ~1e-16).  Needs at least 6 correspondences (a smaller pair never reaches the
    device)."""
    Rt = np.asarray(Rt, np.float64).reshape(3, 4)
    b1 = np.ascontiguousarray(b1, np.float64).reshape(-1, 3)
    if len(b1) < 6:
        raise NotImplementedError("relative_pose_refinement: fewer than 6 correspondences are not refined on the GPU path")
    pose = np.r_[Rt[:, :3].T.reshape(9), -Rt[:, :3].T.dot(Rt[:, 3])]
    res, _, _ = _reconstruction.two_view_pairs(b1, b2, [0, len(b1)], 1.0, poses=pose, refine_iterations=iterations, skip_inlier_tests=True)
    return np.c_[res[0]["R"][0], res[0]["t"][0]]


def _abspose_solve(bearings, points, kind: int, who: str):
    import ctypes as C

    bearings = np.ascontiguousarray(bearings, np.float64).reshape(-1, 3)
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    if len(bearings) != len(points):
        raise ValueError(f"{who}: bearings and points do not agree")
    models, count = np.zeros((4, 3, 4)), C.c_int(0)
    _check(_load().osfm_abspose_solve(_default_context().handle, bearings.ctypes.data_as(C.POINTER(C.c_double)),
                                      points.ctypes.data_as(C.POINTER(C.c_double)), len(bearings), kind,
                                      models.ctypes.data_as(C.POINTER(C.c_double)), C.byref(count)), "osfm_abspose_solve")
    return models, count.value


def absolute_pose_three_points(bearings, points) -> List[np.ndarray]:
    """``geometry::AbsolutePoseThreePoints`` (absolute_pose.h:15-122) on the first three rows: no model or four 3 x 4 models
    [R^T | -R^T t] (a model whose root of the quartic lies outside [-1, 1] is NaN, as in the reference)"""
    models, count = _abspose_solve(bearings, points, 0, "absolute_pose_three_points")
    return [models[i].copy() for i in range(count)]


def absolute_pose_n_points(bearings, points) -> np.ndarray:
    """``geometry::AbsolutePoseNPoints`` (absolute_pose.h:144-189): the 3 x 4 model [R | t] of the Lu-Hager iteration over all rows"""
    models, _ = _abspose_solve(bearings, points, 1, "absolute_pose_n_points")
    return models[0].copy()
