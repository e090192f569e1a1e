"""``pyrobust`` (opensfm/src/robust/python/pybind.cc:26-56): ``ransac_relative_pose`` -- the estimator of the calibrated robust-matching
branch (robust/src/instanciations.cc:33-48) -- and ``ransac_relative_rotation`` -- the estimator that ranks the initial pairs of
``reconstruct`` (instanciations.cc:50-64, through multiview.relative_pose_ransac_rotation_only) -- and ``ransac_absolute_pose`` -- the
estimator of ``resect`` (instanciations.cc:67-83, through multiview.absolute_pose_ransac) -- with ``RobustEstimatorParams`` and
``RansacType``.  The other estimators of the reference's module (line, essential, absolute pose with known rotation, similarity) are
not provided."""
import enum

import numpy as np

from .. import matching as _matching


class RansacType(enum.IntEnum):
    RANSAC = 0
    MSAC = 1
    LMedS = 2


RANSAC, MSAC, LMedS = RansacType.RANSAC, RansacType.MSAC, RansacType.LMedS  # export_values()


class RobustEstimatorParams:
    """robust/robust_estimator.h: iterations 100, probability 0.99, local optimisation (10 iterations) and iteration reduction on"""

    def __init__(self):
        self.iterations = 100
        self.probability = 0.99
        self.use_local_optimization = True
        self.use_iteration_reduction = True
        self.local_optimization_iterations = 10


class ScoreInfoMatrix34d:
    def __init__(self):
        self.score = 0.0
        self.model = np.zeros((3, 4))
        self.lo_model = np.zeros((3, 4))
        self.inliers_indices = []


def ransac_relative_pose(b1, b2, threshold: float, parameters: RobustEstimatorParams, ransac_type: RansacType = RansacType.RANSAC):
    """robust::RANSACRelativePose: LO-RANSAC of the relative pose on unit bearings (n x 3 each); ScoreInfo with the 3 x 4 model [R | t]"""
    if int(ransac_type) != int(RansacType.RANSAC):
        raise NotImplementedError("only RansacType.RANSAC is on the GPU path (what multiview.relative_pose_ransac asks for)")
    if not parameters.use_iteration_reduction:
        raise NotImplementedError("use_iteration_reduction = False is not on the GPU path")
    b1, b2 = np.asarray(b1, np.float64).reshape(-1, 3), np.asarray(b2, np.float64).reshape(-1, 3)
    if len(b1) != len(b2):
        raise RuntimeError("Features matrices have different sizes.")  # instanciations.cc:20-22
    res, mask, _ = _matching.relpose_pairs(b1, b2, [0, len(b1)], threshold, mode="ransac", iterations=parameters.iterations,
                                           probability=parameters.probability, use_lo=parameters.use_local_optimization,
                                           lo_iterations=getattr(parameters, "local_optimization_iterations", 10))
    out = ScoreInfoMatrix34d()
    out.score, out.model, out.lo_model = res[0]["score"], res[0]["model"], res[0]["lo_model"]
    out.inliers_indices = [int(i) for i in np.flatnonzero(mask)]
    return out


class ScoreInfoMatrix3d:
    def __init__(self):
        self.score = 0.0
        self.model = np.zeros((3, 3))
        self.lo_model = np.zeros((3, 3))
        self.inliers_indices = []


def ransac_relative_rotation(b1, b2, threshold: float, parameters: RobustEstimatorParams, ransac_type: RansacType = RansacType.RANSAC):
    """robust::RANSACRelativeRotation: LO-RANSAC of a pure rotation between bearings (n x 3 each, n >= 3); ScoreInfo with the 3 x 3
    model (the rotation from the first bearings to the second, transposed: RotationBetweenPoints(sample)^T)"""
    if int(ransac_type) != int(RansacType.RANSAC):
        raise NotImplementedError("only RansacType.RANSAC is on the GPU path (what multiview.relative_pose_ransac_rotation_only asks for)")
    if not parameters.use_iteration_reduction:
        raise NotImplementedError("use_iteration_reduction = False is not on the GPU path")
    b1, b2 = np.asarray(b1, np.float64).reshape(-1, 3), np.asarray(b2, np.float64).reshape(-1, 3)
    if len(b1) != len(b2):
        raise RuntimeError("Features matrices have different sizes.")  # instanciations.cc:54-56
    from .. import reconstruction as _reconstruction

    res, mask, _ = _reconstruction.relrot_pairs(b1, b2, [0, len(b1)], threshold, iterations=parameters.iterations,
                                                probability=parameters.probability, use_lo=parameters.use_local_optimization,
                                                lo_iterations=getattr(parameters, "local_optimization_iterations", 10))
    out = ScoreInfoMatrix3d()
    out.score, out.model, out.lo_model = float(res[0]["score"]), res[0]["model"], res[0]["lo_model"]
    out.inliers_indices = [int(i) for i in np.flatnonzero(mask)]
    return out


def ransac_absolute_pose(bearings, points, threshold: float, parameters: RobustEstimatorParams, ransac_type: RansacType = RansacType.RANSAC):
    """robust::RANSACAbsolutePose: LO-RANSAC of the camera pose from bearings and points (n x 3 each, n >= 3); ScoreInfo with the 3 x 4
    model [R | t] (world to camera)"""
    if int(ransac_type) != int(RansacType.RANSAC):
        raise NotImplementedError("only RansacType.RANSAC is on the GPU path (what multiview.absolute_pose_ransac asks for)")
    if not parameters.use_iteration_reduction:
        raise NotImplementedError("use_iteration_reduction = False is not on the GPU path")
    bearings, points = np.asarray(bearings, np.float64).reshape(-1, 3), np.asarray(points, np.float64).reshape(-1, 3)
    if len(bearings) != len(points):
        raise RuntimeError("Features matrices have different sizes.")  # instanciations.cc:71-73
    from .. import reconstruction as _reconstruction

    res, mask, _, _ = _reconstruction.abspose_images(bearings, points, [0, len(bearings)], threshold, iterations=parameters.iterations,
                                                     probability=parameters.probability, use_lo=parameters.use_local_optimization,
                                                     lo_iterations=getattr(parameters, "local_optimization_iterations", 10),
                                                     inlier_chord=0.0)
    out = ScoreInfoMatrix34d()
    out.score, out.model, out.lo_model = float(res[0]["score"]), res[0]["model"], res[0]["lo_model"]
    out.inliers_indices = [int(i) for i in np.flatnonzero(mask)]
    return out
