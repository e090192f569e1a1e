"""Drop-ins for the first phase of ``opensfm reconstruct``: ranking the candidate initial pairs (``reconstruction.compute_image_pairs``,
``opensfm/reconstruction.py:208-244``) with one batched rotation-only LO-RANSAC on the GPU (``relrot.hip``).

``compute_image_pairs(track_dict, data)`` takes what ``tracking.all_common_tracks_with_features`` returns, concatenates the pairs'
normalised image coordinates in item order, computes the bearings and runs ``pyrobust.ransac_relative_rotation`` for every pair in
one call, counts the rotation-only inliers and the reconstructability on the device, and sorts on the host exactly as the reference
does (``np.argsort(-np.array(score))``).

``triangulate_shot_features(tracks_manager, reconstruction, shot_ids, config)`` and ``retriangulate(tracks_manager, reconstruction, config)``
(``reconstruction.py:1143-1226``) triangulate every track of their batch in one GPU call (``triangulate.hip``, ``triangulation_type: FULL``, or ``ROBUST`` when ``robust_seed`` or ``robust_draws`` says where the draws come from);
``triangulate_bearings_arrays`` / ``triangulate_tracks_arrays`` and their ``_robust`` forms are the same calls on flat arrays.

``resect(data, tracks_manager, reconstruction, shot_id, threshold, min_inliers)`` (``reconstruction.py:695-762``) adds one image to the map
with the absolute-pose LO-RANSAC of ``abspose.hip``; ``resect_candidates`` is the candidate loop of ``grow_reconstruction``
(``:1525-1575``) with up to ``max_batch`` candidates solved per GPU call; ``abspose_images`` / ``abspose_images_pixels`` are the same
estimator on flat arrays and ``absolute_pose_ransac`` is ``multiview.absolute_pose_ransac``.

``cull_final_point_cloud(reconstruction, config)`` is the tail of ``grow_reconstruction`` after its last bundle
(``reconstruction.py:1586-1594``): the outlier step (``discard_gross_observations``) and, under ``filter_final_point_cloud``, the two point-cloud filters on the GPU
(``cloud.hip``).

``two_view_reconstruction_general(p1, p2, camera1, camera2, threshold, iterations, check_reversal, reversal_ratio)``
(``reconstruction.py:488-560``) turns a ranked pair into the first two poses: bearings, 5-point LO-RANSAC, both configurations of
``two_view_reconstruction_5pt`` and the choice between them in one GPU call (``twoview.hip``); ``two_view_reconstruction_general_pairs`` does
that for the first K ranked pairs at once, ``two_view_pairs`` / ``two_view_pairs_pixels`` are the same calls on flat arrays, and
``two_view_reconstruction_and_refinement`` / ``two_view_reconstruction_5pt`` are the reference's functions on given poses.  The
plane-based branch (``two_view_reconstruction_plane_based``, ``reconstruction.py:298-333``) runs on the GPU too (``plane.hip``) when
``plane_based="device"`` is passed: one more call for the whole list; ``two_view_plane_pairs`` / ``two_view_plane_pairs_pixels`` are that
call on flat arrays and ``motion_from_plane_homography`` is ``multiview.motion_from_plane_homography``."""
from __future__ import annotations

import ctypes as C
import time
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence, Set, Tuple

import numpy as np

from ._lib import (AbsposeParams, AbsposeResult, PlaneParams, PlaneResult, RelrotParams, RelrotResult, TriangulateParams, TwoViewParams,
                   TwoViewResult, check, default_context, load)
from .matching import camera_parameters


def _fptr(a: np.ndarray, t):
    return a.ctypes.data_as(C.POINTER(t))


def _params(threshold: float, iterations: int, probability: float, use_lo: bool, lo_iterations: int, use_iteration_reduction: bool,
            inlier_chord: float) -> RelrotParams:
    return RelrotParams(float(threshold), float(probability), float(inlier_chord), int(iterations), int(bool(use_lo)), int(lo_iterations),
                        int(bool(use_iteration_reduction)))


def _results(res, n_pairs: int) -> List[Dict[str, Any]]:
    out = []
    for p in range(n_pairs):
        r = res[p]
        out.append({"model": np.array(r.model).reshape(3, 3), "lo_model": np.array(r.lo_model).reshape(3, 3), "score": r.score,
                    "iterations": r.iterations, "n_rotation_inliers": r.n_rotation_inliers, "reconstructability": r.reconstructability})
    return out


def relrot_pairs(b1: np.ndarray, b2: np.ndarray, offsets: Sequence[int], threshold: float, iterations: int = 1000, probability: float = 0.99,
                 use_lo: bool = True, lo_iterations: int = 10, use_iteration_reduction: bool = True, inlier_chord: float = 0.0,
                 ctx=None) -> Tuple[List[Dict[str, Any]], np.ndarray, float]:
    """Batched ``pyrobust.ransac_relative_rotation`` on bearings (``osfm_relrot_pairs``): pair p owns rows offsets[p]:offsets[p+1] of
    b1 / b2.  -> (per-pair dicts, mask of the RANSAC inliers over all rows, kernel milliseconds)."""
    ctx = ctx or default_context()
    b1 = np.ascontiguousarray(b1, np.float64).reshape(-1, 3)
    b2 = np.ascontiguousarray(b2, np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(offsets, np.int64)
    n_pairs = len(off) - 1
    if len(b1) != len(b2) or n_pairs < 0 or (n_pairs > 0 and off[-1] != len(b1)):
        raise ValueError("relrot_pairs: b1 / b2 / offsets do not agree")
    prm = _params(threshold, iterations, probability, use_lo, lo_iterations, use_iteration_reduction, inlier_chord)
    res = (RelrotResult * max(n_pairs, 1))()
    mask = np.zeros(max(len(b1), 1), np.uint8)
    ms = C.c_double(0.0)
    check(load().osfm_relrot_pairs(ctx.handle, _fptr(b1, C.c_double), _fptr(b2, C.c_double), _fptr(off, C.c_int64), n_pairs, C.byref(prm), res,
                                   _fptr(mask, C.c_uint8), C.byref(ms)), "osfm_relrot_pairs")
    return _results(res, n_pairs), mask[: len(b1)].astype(bool), ms.value


def relrot_pairs_pixels(p1: np.ndarray, p2: np.ndarray, offsets: Sequence[int], pair_cams: np.ndarray, cam_model: np.ndarray,
                        cam_params: np.ndarray, threshold: float, iterations: int = 1000, probability: float = 0.99, use_lo: bool = True,
                        lo_iterations: int = 10, inlier_chord: float = 0.0, with_mask: bool = False,
                        ctx=None) -> Tuple[List[Dict[str, Any]], Optional[np.ndarray], float]:
    """``osfm_relrot_pairs_pixels``: the same from normalised image coordinates, the bearings computed on the device with the cameras
    pair_cams[p] = (camera of side 1, camera of side 2) of the table cam_model (n_cams) / cam_params (n_cams x 16)."""
    ctx = ctx or default_context()
    p1 = np.ascontiguousarray(np.asarray(p1, np.float64)[:, :2])
    p2 = np.ascontiguousarray(np.asarray(p2, np.float64)[:, :2])
    off = np.ascontiguousarray(offsets, np.int64)
    n_pairs = len(off) - 1
    if len(p1) != len(p2) or n_pairs < 0 or (n_pairs > 0 and off[-1] != len(p1)):
        raise ValueError("relrot_pairs_pixels: p1 / p2 / offsets do not agree")
    pc = np.ascontiguousarray(pair_cams, np.int32)
    cm = np.ascontiguousarray(cam_model, np.int32)
    cp = np.ascontiguousarray(cam_params, np.float64)
    if pc.shape != (n_pairs, 2) or cm.ndim != 1 or cp.shape != (len(cm), 16):
        raise ValueError(f"relrot_pairs_pixels: pair_cams must be ({n_pairs}, 2) and cam_params ({len(cm)}, 16) for cam_model of length "
                         f"{len(cm)}; got {pc.shape}, {cp.shape}")
    prm = _params(threshold, iterations, probability, use_lo, lo_iterations, True, inlier_chord)
    res = (RelrotResult * max(n_pairs, 1))()
    mask = np.zeros(max(len(p1), 1), np.uint8) if with_mask else None
    ms = C.c_double(0.0)
    check(load().osfm_relrot_pairs_pixels(ctx.handle, _fptr(p1, C.c_double), _fptr(p2, C.c_double), _fptr(off, C.c_int64), n_pairs,
                                          _fptr(pc, C.c_int32), _fptr(cm, C.c_int32), _fptr(cp, C.c_double), len(cm), C.byref(prm), res,
                                          _fptr(mask, C.c_uint8) if with_mask else None, C.byref(ms)), "osfm_relrot_pairs_pixels")
    return _results(res, n_pairs), (mask[: len(p1)].astype(bool) if with_mask else None), ms.value


def pairwise_reconstructability(common_tracks: int, rotation_inliers: int) -> float:
    """Likeliness of an image pair giving a good initial reconstruction (``reconstruction.py:193-200``)."""
    outliers = common_tracks - rotation_inliers
    outlier_ratio = float(outliers) / common_tracks
    if outlier_ratio >= 0.3:
        return outliers
    else:
        return 0


def _camera_table(track_dict, data) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """pair_cams (n_pairs x 2), cam_model, cam_params of the cameras the pairs' images use (``_pair_reconstructability_arguments``)."""
    cameras = data.load_camera_models()
    index: Dict[str, int] = {}
    models: List[int] = []
    params: List[np.ndarray] = []
    pair_cams = np.zeros((len(track_dict), 2), np.int32)
    for k, (im1, im2) in enumerate(track_dict.keys()):
        for side, im in enumerate((im1, im2)):
            key = data.load_exif(im)["camera"]
            if key not in index:
                model, par = camera_parameters(cameras[key])
                index[key] = len(models)
                models.append(model)
                params.append(par)
            pair_cams[k, side] = index[key]
    return pair_cams, np.array(models, np.int32), np.array(params, np.float64).reshape(-1, 16)


def compute_image_pairs(track_dict: Dict[Tuple[str, str], Any], data, ctx=None) -> List[Tuple[str, str]]:
    """All matched image pairs sorted by reconstructability (``reconstruction.py:208-220``): same arguments, same return."""
    if not track_dict:
        return []
    threshold = 4 * data.config["five_point_algo_threshold"]
    pair_cams, cam_model, cam_params = _camera_table(track_dict, data)
    values = list(track_dict.values())
    p1 = np.concatenate([np.asarray(v[1], np.float64).reshape(-1, 2) for v in values])
    p2 = np.concatenate([np.asarray(v[2], np.float64).reshape(-1, 2) for v in values])
    off = np.r_[0, np.cumsum([len(v[1]) for v in values])].astype(np.int64)
    # two_view_reconstruction_rotation_only: relative_pose_ransac_rotation_only(b1, b2, threshold, 1000, 0.999) -- the 0.999 is not
    # passed on (multiview.py:520-540 sets only the iterations), so the probability is the default 0.99
    res, _, _ = relrot_pairs_pixels(p1, p2, off, pair_cams, cam_model, cam_params, threshold, iterations=1000, probability=0.99, use_lo=True,
                                    lo_iterations=10, inlier_chord=threshold, ctx=ctx)
    keys = list(track_dict.keys())
    pairs = [keys[k] for k, r in enumerate(res) if r["reconstructability"] > 0]
    score = [int(r["reconstructability"]) for r in res if r["reconstructability"] > 0]
    order = np.argsort(-np.array(score))
    return [pairs[o] for o in order]


def _residual_table(landmarks) -> Tuple[List[Tuple[str, str]], np.ndarray]:
    """every reprojection error the last bundle stored on the landmarks: its (landmark id, shot id) and the errors as rows of one array"""
    keys = [(lm_id, shot_id) for lm_id, lm in landmarks.items() for shot_id in lm.reprojection_errors]
    rows = np.array([landmarks[lm_id].reprojection_errors[shot_id] for lm_id, shot_id in keys], np.float64)
    return keys, rows.reshape(len(keys), -1) if keys else np.zeros((0, 2))


def _residual_limit(config: Dict[str, Any], rows: np.ndarray) -> float:
    """the largest reprojection error an observation may keep.  ``bundle_outlier_filtering_type`` FIXED: the configured constant.  AUTO: a
    robust scale of all residuals -- the componentwise median m, 1.486 times the median distance to it as the spread s, and
    ``bundle_outlier_auto_ratio`` * |m + s|.  Anything else: 1.  A missing key is a KeyError, as in the reference."""
    mode = config["bundle_outlier_filtering_type"]
    if mode == "FIXED":
        return float(config["bundle_outlier_fixed_threshold"])
    if mode == "AUTO":
        centre = np.median(rows, axis=0)
        spread = 1.486 * np.median(np.sqrt(((rows - centre) ** 2).sum(axis=1)))
        return float(config["bundle_outlier_auto_ratio"]) * float(np.linalg.norm(centre + spread))
    return 1.0


def discard_gross_observations(reconstruction, config: Dict[str, Any]) -> int:
    """The outlier step after a bundle, with the result of the reference's ``remove_outliers`` (which itself runs unmodified on
    ``geometry_types.Reconstruction``; this one is for callers that do not load the reference's module).  One vectorised pass over the
    table of stored reprojection errors: an observation whose first two error components exceed the limit in norm leaves its shot, and a
    landmark that lost one and has fewer than two left leaves the map.  Returns the number of observations discarded."""
    landmarks = reconstruction.points
    keys, rows = _residual_table(landmarks)
    if not keys:
        return 0
    limit = _residual_limit(config, rows)
    gross = np.flatnonzero(rows[:, 0] ** 2 + rows[:, 1] ** 2 > limit * limit)
    thinned = dict.fromkeys(keys[i][0] for i in gross)  # in first-hit order, each once
    for i in gross:
        lm_id, shot_id = keys[i]
        reconstruction.map.remove_observation(shot_id, lm_id)
    for lm_id in thinned:
        if landmarks[lm_id].number_of_observations() < 2:
            reconstruction.map.remove_landmark(landmarks[lm_id])
    return len(gross)


def cull_final_point_cloud(reconstruction, config: Dict[str, Any]) -> Dict[str, int]:
    """What ``grow_reconstruction`` does after its final bundle, for callers that do not load the reference's module: the outlier step and,
    if ``config["filter_final_point_cloud"]``, ``pysfm.filter_badly_conditioned_points`` with ``config["triangulation_min_ray_angle"]``
    and ``pysfm.remove_isolated_points``.  The keys are read as the reference reads them: a missing one is a KeyError.  Returns what each
    step removed."""
    from . import opensfm_adapter

    report = {"outlier_observations": discard_gross_observations(reconstruction, config), "badly_conditioned": 0, "isolated": 0}
    if config["filter_final_point_cloud"]:
        report["badly_conditioned"] = opensfm_adapter.filter_badly_conditioned_points(reconstruction.map, config["triangulation_min_ray_angle"])
        report["isolated"] = opensfm_adapter.remove_isolated_points(reconstruction.map)
    return report


# ------------------------------------------------------------------------------------------------
# triangulation of tracks (reconstruction.py:1032-1226)
# ------------------------------------------------------------------------------------------------
TRIANGULATION_STATUS = ("triangulated", "fewer than 2 observations", "ray angle", "reprojection angle", "depth", "result not finite",
                        "no consensus")  # (2 .. 4: FULL only; 6: ROBUST only)
ROBUST_TRIES = 11


def _triangulate_params(threshold: float, min_angle_deg: float, min_depth: float, refinement_iterations: int) -> TriangulateParams:
    return TriangulateParams(float(threshold), float(min_angle_deg), float(min_depth), int(refinement_iterations), 0)


def _triangulate_outputs(n_tracks: int):
    return np.full((max(n_tracks, 1), 3), np.nan), np.zeros(max(n_tracks, 1), np.uint8), np.zeros(max(n_tracks, 1), np.int32), C.c_double(0.0)


def triangulate_bearings_arrays(centers: np.ndarray, bearings: np.ndarray, track_offsets: Sequence[int], threshold: float = 0.006,
                                min_angle_deg: float = 1.0, min_depth: float = 0.001, refinement_iterations: int = 10,
                                ctx=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, float]:
    """``osfm_triangulate_bearings``: track t owns rows track_offsets[t]:track_offsets[t+1] of centers / bearings (world coordinates).
    -> (points (n, 3), NaN unless triangulated; status (n,), see TRIANGULATION_STATUS; TinySolver iterations (n,); kernel milliseconds)."""
    ctx = ctx or default_context()
    centers = np.ascontiguousarray(centers, np.float64).reshape(-1, 3)
    bearings = np.ascontiguousarray(bearings, np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(track_offsets, np.int64)
    n_tracks = len(off) - 1
    if len(centers) != len(bearings) or n_tracks < 0 or (n_tracks > 0 and off[-1] != len(centers)):
        raise ValueError("triangulate_bearings_arrays: centers / bearings / track_offsets do not agree")
    prm = _triangulate_params(threshold, min_angle_deg, min_depth, refinement_iterations)
    points, status, iterations, ms = _triangulate_outputs(n_tracks)
    check(load().osfm_triangulate_bearings(ctx.handle, _fptr(centers, C.c_double), _fptr(bearings, C.c_double), _fptr(off, C.c_int64), n_tracks,
                                           C.byref(prm), _fptr(points, C.c_double), _fptr(status, C.c_uint8), _fptr(iterations, C.c_int32),
                                           C.byref(ms)), "osfm_triangulate_bearings")
    return points[:n_tracks], status[:n_tracks], iterations[:n_tracks], ms.value


def triangulate_tracks_arrays(shot_pose: np.ndarray, shot_camera: np.ndarray, cam_model: np.ndarray, cam_params: np.ndarray,
                              obs_shot: np.ndarray, obs_xy: np.ndarray, track_offsets: Sequence[int], threshold: float = 0.006,
                              min_angle_deg: float = 1.0, min_depth: float = 0.001, refinement_iterations: int = 10,
                              ctx=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, float]:
    """``osfm_triangulate_tracks``: the same from (shot, normalised image point) rows; shot_pose (n_shots, 12) holds R (row-major) then t
    of every shot's world-to-camera pose composed with its rig, cam_params (n_cams, 16) the cameras in the native parameter order."""
    ctx = ctx or default_context()
    shot_pose = np.ascontiguousarray(shot_pose, np.float64).reshape(-1, 12)
    shot_camera = np.ascontiguousarray(shot_camera, np.int32)
    cam_model = np.ascontiguousarray(cam_model, np.int32)
    cam_params = np.ascontiguousarray(cam_params, np.float64).reshape(-1, 16)
    obs_shot = np.ascontiguousarray(obs_shot, np.int32)
    obs_xy = np.ascontiguousarray(np.asarray(obs_xy, np.float64).reshape(-1, 2))
    off = np.ascontiguousarray(track_offsets, np.int64)
    n_tracks = len(off) - 1
    if (len(shot_camera) != len(shot_pose) or len(cam_params) != len(cam_model) or len(obs_shot) != len(obs_xy) or n_tracks < 0
            or (n_tracks > 0 and off[-1] != len(obs_shot))):
        raise ValueError("triangulate_tracks_arrays: array lengths do not agree")
    prm = _triangulate_params(threshold, min_angle_deg, min_depth, refinement_iterations)
    points, status, iterations, ms = _triangulate_outputs(n_tracks)
    check(load().osfm_triangulate_tracks(ctx.handle, _fptr(shot_pose, C.c_double), _fptr(shot_camera, C.c_int32), len(shot_pose),
                                         _fptr(cam_model, C.c_int32), _fptr(cam_params, C.c_double), len(cam_model), _fptr(obs_shot, C.c_int32),
                                         _fptr(obs_xy, C.c_double), _fptr(off, C.c_int64), n_tracks, C.byref(prm), _fptr(points, C.c_double),
                                         _fptr(status, C.c_uint8), _fptr(iterations, C.c_int32), C.byref(ms)), "osfm_triangulate_tracks")
    return points[:n_tracks], status[:n_tracks], iterations[:n_tracks], ms.value


def _robust_draws(draws, n_tracks: int, who: str):
    """-> (the (n_tracks, 11) float64 array or None, its pointer or a null one)"""
    if draws is None:
        return None, C.POINTER(C.c_double)()
    draws = np.ascontiguousarray(draws, np.float64).reshape(-1, ROBUST_TRIES)
    if len(draws) != n_tracks:
        raise ValueError(who + ": draws must be n_tracks x %d" % ROBUST_TRIES)
    return draws, _fptr(draws, C.c_double)


def _robust_outputs(n_tracks: int, n_obs: int):
    return (np.full((max(n_tracks, 1), 3), np.nan), np.zeros(max(n_tracks, 1), np.uint8), np.zeros(max(n_obs, 1), np.uint8),
            np.zeros(max(n_tracks, 1), np.int32), np.zeros(max(n_tracks, 1), np.int32), C.c_double(0.0))


def triangulate_bearings_arrays_robust(centers: np.ndarray, bearings: np.ndarray, track_offsets: Sequence[int], threshold: float = 0.006,
                                       min_angle_deg: float = 1.0, min_depth: float = 0.001, refinement_iterations: int = 10, draws=None,
                                       seed: int = 0, ctx=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, float]:
    """``osfm_triangulate_bearings_robust`` (TrackTriangulator.triangulate_robust per track): `draws` (n_tracks, 11) in [0, 1), or None for
    the library's generator over (seed, track, try).  -> (points (n, 3), NaN unless triangulated; status (n,): 0, 1, 5 or 6 of
    TRIANGULATION_STATUS; inlier_mask (n_obs,) uint8; n_inliers (n,); tries_used (n,); kernel milliseconds)."""
    ctx = ctx or default_context()
    centers = np.ascontiguousarray(centers, np.float64).reshape(-1, 3)
    bearings = np.ascontiguousarray(bearings, np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(track_offsets, np.int64)
    n_tracks = len(off) - 1
    if len(centers) != len(bearings) or n_tracks < 0 or (n_tracks > 0 and off[-1] != len(centers)):
        raise ValueError("triangulate_bearings_arrays_robust: centers / bearings / track_offsets do not agree")
    draws, draws_ptr = _robust_draws(draws, n_tracks, "triangulate_bearings_arrays_robust")
    prm = _triangulate_params(threshold, min_angle_deg, min_depth, refinement_iterations)
    points, status, mask, n_inliers, tries, ms = _robust_outputs(n_tracks, len(centers))
    check(load().osfm_triangulate_bearings_robust(ctx.handle, _fptr(centers, C.c_double), _fptr(bearings, C.c_double), _fptr(off, C.c_int64),
                                                  n_tracks, C.byref(prm), draws_ptr, C.c_uint64(int(seed) & (2**64 - 1)), _fptr(points, C.c_double),
                                                  _fptr(status, C.c_uint8), _fptr(mask, C.c_uint8), _fptr(n_inliers, C.c_int32),
                                                  _fptr(tries, C.c_int32), C.byref(ms)), "osfm_triangulate_bearings_robust")
    return points[:n_tracks], status[:n_tracks], mask[:len(centers)], n_inliers[:n_tracks], tries[:n_tracks], ms.value


def triangulate_tracks_arrays_robust(shot_pose: np.ndarray, shot_camera: np.ndarray, cam_model: np.ndarray, cam_params: np.ndarray,
                                     obs_shot: np.ndarray, obs_xy: np.ndarray, track_offsets: Sequence[int], threshold: float = 0.006,
                                     min_angle_deg: float = 1.0, min_depth: float = 0.001, refinement_iterations: int = 10, draws=None,
                                     seed: int = 0, ctx=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, float]:
    """``osfm_triangulate_tracks_robust``: the same from (shot, normalised image point) rows, the tables as for triangulate_tracks_arrays."""
    ctx = ctx or default_context()
    shot_pose = np.ascontiguousarray(shot_pose, np.float64).reshape(-1, 12)
    shot_camera = np.ascontiguousarray(shot_camera, np.int32)
    cam_model = np.ascontiguousarray(cam_model, np.int32)
    cam_params = np.ascontiguousarray(cam_params, np.float64).reshape(-1, 16)
    obs_shot = np.ascontiguousarray(obs_shot, np.int32)
    obs_xy = np.ascontiguousarray(np.asarray(obs_xy, np.float64).reshape(-1, 2))
    off = np.ascontiguousarray(track_offsets, np.int64)
    n_tracks = len(off) - 1
    if (len(shot_camera) != len(shot_pose) or len(cam_params) != len(cam_model) or len(obs_shot) != len(obs_xy) or n_tracks < 0
            or (n_tracks > 0 and off[-1] != len(obs_shot))):
        raise ValueError("triangulate_tracks_arrays_robust: array lengths do not agree")
    draws, draws_ptr = _robust_draws(draws, n_tracks, "triangulate_tracks_arrays_robust")
    prm = _triangulate_params(threshold, min_angle_deg, min_depth, refinement_iterations)
    points, status, mask, n_inliers, tries, ms = _robust_outputs(n_tracks, len(obs_shot))
    check(load().osfm_triangulate_tracks_robust(ctx.handle, _fptr(shot_pose, C.c_double), _fptr(shot_camera, C.c_int32), len(shot_pose),
                                                _fptr(cam_model, C.c_int32), _fptr(cam_params, C.c_double), len(cam_model),
                                                _fptr(obs_shot, C.c_int32), _fptr(obs_xy, C.c_double), _fptr(off, C.c_int64), n_tracks,
                                                C.byref(prm), draws_ptr, C.c_uint64(int(seed) & (2**64 - 1)), _fptr(points, C.c_double),
                                                _fptr(status, C.c_uint8), _fptr(mask, C.c_uint8), _fptr(n_inliers, C.c_int32),
                                                _fptr(tries, C.c_int32), C.byref(ms)), "osfm_triangulate_tracks_robust")
    return points[:n_tracks], status[:n_tracks], mask[:len(obs_shot)], n_inliers[:n_tracks], tries[:n_tracks], ms.value


def _triangulate_into(tracks_manager, reconstruction, track_ids: List[str], config: Dict[str, Any], ctx=None, *, robust_seed=None,
                      robust_draws=None) -> None:
    """TrackTriangulator.triangulate for every track of `track_ids` in one call: the observations of a track in the shots of the
    reconstruction, in the order the manager returns them; every accepted track becomes a point that all of them observe.
    ``triangulation_type: ROBUST`` is TrackTriangulator.triangulate_robust in one call, and needs to be told where its draws come from:
    `robust_seed` (the library's generator; track k of `track_ids` draws as track k) or `robust_draws` (len(track_ids) x 11 values in
    [0, 1), row k for track k).  Only a track's best inliers then observe its point."""
    threshold = config["triangulation_threshold"]
    min_ray_angle = config["triangulation_min_ray_angle"]
    min_depth = config["triangulation_min_depth"]
    refinement_iterations = config["triangulation_refinement_iterations"]
    kind = config["triangulation_type"]
    robust = kind == "ROBUST"
    if robust and robust_seed is None and robust_draws is None:
        raise NotImplementedError("triangulation_type ROBUST draws from numpy's global generator over an unordered set of tracks in the "
                                  "reference: it has no reproducible result there.  Pass robust_seed= (the library's per-track generator) "
                                  "or robust_draws= (len(track_ids) x 11 values in [0, 1)) to run it on the GPU")
    if robust and robust_seed is not None and robust_draws is not None:
        raise ValueError("robust_seed and robust_draws exclude each other")
    if robust and robust_draws is not None:
        robust_draws = np.asarray(robust_draws, np.float64).reshape(-1, ROBUST_TRIES)
        if len(robust_draws) != len(track_ids):
            raise ValueError("robust_draws must hold %d values for each of the call's %d tracks" % (ROBUST_TRIES, len(track_ids)))
    if kind not in ("FULL", "ROBUST") or not track_ids:  # (the reference does nothing for any other value)
        return
    shots = reconstruction.shots
    shot_index: Dict[str, int] = {}
    cam_index: Dict[str, int] = {}
    poses: List[np.ndarray] = []
    shot_camera: List[int] = []
    models: List[int] = []
    params: List[np.ndarray] = []
    obs_shot: List[int] = []
    obs_xy: List[Any] = []
    members: List[List[str]] = []
    for track in track_ids:
        ids = []
        for shot_id, obs in tracks_manager.get_track_observations(track).items():
            if shot_id not in shots:
                continue
            s = shot_index.get(shot_id)
            if s is None:
                shot = shots[shot_id]
                cam = shot.camera
                if cam.id not in cam_index:
                    model, par = camera_parameters(cam)
                    cam_index[cam.id] = len(models)
                    models.append(model)
                    params.append(par)
                pose = shot.pose
                poses.append(np.r_[np.asarray(pose.get_rotation_matrix(), float).reshape(9), np.asarray(pose.translation, float).reshape(3)])
                shot_camera.append(cam_index[cam.id])
                s = shot_index[shot_id] = len(poses) - 1
            obs_shot.append(s)
            obs_xy.append(obs.point)
            ids.append(shot_id)
        members.append(ids)
    offsets = np.r_[0, np.cumsum([len(m) for m in members])].astype(np.int64)
    if not poses:  # no track has an observation in the reconstruction
        return
    tables = (np.array(poses), np.array(shot_camera, np.int32), np.array(models, np.int32), np.array(params, np.float64).reshape(-1, 16),
              np.array(obs_shot, np.int32), np.array(obs_xy, np.float64).reshape(-1, 2), offsets, threshold, min_ray_angle, min_depth,
              refinement_iterations)
    if robust:
        points, status, mask, _, _, _ = triangulate_tracks_arrays_robust(*tables, draws=robust_draws, seed=robust_seed or 0, ctx=ctx)
    else:
        points, status, _, _ = triangulate_tracks_arrays(*tables, ctx=ctx)
        mask = np.ones(len(obs_shot), np.uint8)
    for k, (track, ids, X, st) in enumerate(zip(track_ids, members, points, status)):
        if st != 0:
            continue
        reconstruction.create_point(track, X.tolist())
        for shot_id, inlier in zip(ids, mask[offsets[k]:offsets[k + 1]]):
            if inlier:
                reconstruction.add_observation(shot_id, track, tracks_manager.get_observation(shot_id, track))


def triangulate_shot_features(tracks_manager, reconstruction, shot_ids, config: Dict[str, Any], ctx=None, *, robust_seed=None,
                              robust_draws=None) -> None:
    """Reconstruct as many tracks seen in `shot_ids` as possible (``reconstruction.py:1143-1183``): the tracks of those shots that the
    reconstruction does not hold yet, one GPU call.  ``triangulation_type`` FULL, or ROBUST with `robust_seed` or `robust_draws` (see
    _triangulate_into; the call's track list is the tracks of `shot_ids` in the given order of the shots, each shot's in the manager's
    order, first sighting, minus the points the map holds); ROBUST with neither raises NotImplementedError."""
    all_shots_ids = set(tracks_manager.get_shot_ids())
    tracks_ids = dict.fromkeys(t for s in shot_ids if s in all_shots_ids for t in tracks_manager.get_shot_observations(s))
    _triangulate_into(tracks_manager, reconstruction, [t for t in tracks_ids if t not in reconstruction.points], config, ctx,
                      robust_seed=robust_seed, robust_draws=robust_draws)


def retriangulate(tracks_manager, reconstruction, config: Dict[str, Any], ctx=None, *, robust_seed=None, robust_draws=None) -> Dict[str, Any]:
    """Retriangulate all points (``reconstruction.py:1186-1226``): the map's points are dropped and every track seen by its shots goes
    through one GPU call (the track list: the tracks of the reconstruction's shots in map order, first sighting).  ROBUST as for
    triangulate_shot_features.  -> {"num_points_before", "num_points_after", "wall_time"}"""
    start = time.perf_counter()
    report: Dict[str, Any] = {"num_points_before": len(reconstruction.points)}
    for key in ("triangulation_threshold", "triangulation_min_ray_angle", "triangulation_min_depth", "triangulation_refinement_iterations"):
        config[key]  # read before the map is touched, as the reference does
    if config["triangulation_type"] == "ROBUST" and robust_seed is None and robust_draws is None:
        _triangulate_into(tracks_manager, reconstruction, [], config, ctx)  # raises
    if hasattr(reconstruction, "remove_landmark"):
        for lm_id in list(reconstruction.points):
            reconstruction.remove_landmark(lm_id)
    else:
        reconstruction.points = {}
    all_shots_ids = set(tracks_manager.get_shot_ids())
    tracks = dict.fromkeys(t for image in reconstruction.shots.keys() if image in all_shots_ids
                           for t in tracks_manager.get_shot_observations(image).keys())
    _triangulate_into(tracks_manager, reconstruction, list(tracks), config, ctx, robust_seed=robust_seed, robust_draws=robust_draws)
    report["num_points_after"] = len(reconstruction.points)
    report["wall_time"] = time.perf_counter() - start
    return report


# ------------------------------------------------------------------------------------------------
# resection of candidate images (reconstruction.py:677-762, 1525-1575)
# ------------------------------------------------------------------------------------------------
def _abspose_params(threshold: float, iterations: int, probability: float, use_lo: bool, lo_iterations: int, use_iteration_reduction: bool,
                    inlier_chord: Optional[float]) -> AbsposeParams:
    chord = threshold if inlier_chord is None else inlier_chord
    return AbsposeParams(float(threshold), float(probability), float(chord), int(iterations), int(bool(use_lo)), int(lo_iterations),
                         int(bool(use_iteration_reduction)))


def _abspose_results(res, n_images: int) -> List[Dict[str, Any]]:
    return [{"model": np.array(res[i].model).reshape(3, 4), "lo_model": np.array(res[i].lo_model).reshape(3, 4), "score": res[i].score,
             "iterations": res[i].iterations, "num_inliers": res[i].num_inliers} for i in range(n_images)]


def abspose_images(bearings: np.ndarray, points: np.ndarray, offsets: Sequence[int], threshold: float, iterations: int = 1000,
                   probability: float = 0.99, use_lo: bool = True, lo_iterations: int = 10, use_iteration_reduction: bool = True,
                   inlier_chord: Optional[float] = None, ctx=None) -> Tuple[List[Dict[str, Any]], np.ndarray, np.ndarray, float]:
    """Batched ``pyrobust.ransac_absolute_pose`` on bearings and points (``osfm_abspose_images``): image i owns rows
    offsets[i]:offsets[i+1].  ``inlier_chord``: the chord of ``resect``'s inlier test on the inverted lo_model (default: the threshold;
    <= 0 skips it).  -> (per-image dicts, mask of the RANSAC inliers, mask of resect's inliers, kernel milliseconds)."""
    ctx = ctx or default_context()
    b = np.ascontiguousarray(bearings, np.float64).reshape(-1, 3)
    X = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(offsets, np.int64)
    n_images = len(off) - 1
    if len(b) != len(X) or n_images < 0 or (n_images > 0 and off[-1] != len(b)):
        raise ValueError("abspose_images: bearings / points / offsets do not agree")
    prm = _abspose_params(threshold, iterations, probability, use_lo, lo_iterations, use_iteration_reduction, inlier_chord)
    res = (AbsposeResult * max(n_images, 1))()
    rmask, cmask = np.zeros(max(len(b), 1), np.uint8), np.zeros(max(len(b), 1), np.uint8)
    ms = C.c_double(0.0)
    check(load().osfm_abspose_images(ctx.handle, _fptr(b, C.c_double), _fptr(X, C.c_double), _fptr(off, C.c_int64), n_images, C.byref(prm), res,
                                     _fptr(rmask, C.c_uint8), _fptr(cmask, C.c_uint8), C.byref(ms)), "osfm_abspose_images")
    return _abspose_results(res, n_images), rmask[: len(b)].astype(bool), cmask[: len(b)].astype(bool), ms.value


def abspose_images_pixels(xy: np.ndarray, points: np.ndarray, offsets: Sequence[int], image_cam: np.ndarray, cam_model: np.ndarray,
                          cam_params: np.ndarray, threshold: float, iterations: int = 1000, probability: float = 0.99, use_lo: bool = True,
                          lo_iterations: int = 10, use_iteration_reduction: bool = True, inlier_chord: Optional[float] = None,
                          ctx=None) -> Tuple[List[Dict[str, Any]], np.ndarray, np.ndarray, float]:
    """``osfm_abspose_images_pixels``: the same from normalised image coordinates, the bearings computed on the device with camera
    image_cam[i] of the table cam_model (n_cams) / cam_params (n_cams x 16)."""
    ctx = ctx or default_context()
    xy = np.ascontiguousarray(np.asarray(xy, np.float64).reshape(-1, 2))
    X = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(offsets, np.int64)
    n_images = len(off) - 1
    if len(xy) != len(X) or n_images < 0 or (n_images > 0 and off[-1] != len(xy)):
        raise ValueError("abspose_images_pixels: xy / points / offsets do not agree")
    ic = np.ascontiguousarray(image_cam, np.int32)
    cm = np.ascontiguousarray(cam_model, np.int32)
    cp = np.ascontiguousarray(cam_params, np.float64)
    if ic.shape != (n_images,) or cm.ndim != 1 or cp.shape != (len(cm), 16):
        raise ValueError(f"abspose_images_pixels: image_cam must be ({n_images},) and cam_params ({len(cm)}, 16) for cam_model of length "
                         f"{len(cm)}; got {ic.shape}, {cp.shape}")
    prm = _abspose_params(threshold, iterations, probability, use_lo, lo_iterations, use_iteration_reduction, inlier_chord)
    res = (AbsposeResult * max(n_images, 1))()
    rmask, cmask = np.zeros(max(len(xy), 1), np.uint8), np.zeros(max(len(xy), 1), np.uint8)
    ms = C.c_double(0.0)
    check(load().osfm_abspose_images_pixels(ctx.handle, _fptr(xy, C.c_double), _fptr(X, C.c_double), _fptr(off, C.c_int64), n_images,
                                            _fptr(ic, C.c_int32), _fptr(cm, C.c_int32), _fptr(cp, C.c_double), len(cm), C.byref(prm), res,
                                            _fptr(rmask, C.c_uint8), _fptr(cmask, C.c_uint8), C.byref(ms)), "osfm_abspose_images_pixels")
    return _abspose_results(res, n_images), rmask[: len(xy)].astype(bool), cmask[: len(xy)].astype(bool), ms.value


def _invert_model(lo_model: np.ndarray) -> np.ndarray:
    Rt = lo_model.copy()  # multiview.py:487-491
    R, t = Rt[:3, :3].copy(), Rt[:, 3].copy()
    Rt[:3, :3] = R.T
    Rt[:, 3] = -R.T.dot(t)
    return Rt


def absolute_pose_ransac(bs: np.ndarray, Xs: np.ndarray, threshold: float, iterations: int, probability: float, ctx=None) -> np.ndarray:
    """``multiview.absolute_pose_ransac`` (``multiview.py:468-491``): the inverted lo_model, [R^T | -R^T t]."""
    # only the iterations are passed on (multiview.py:475-476 sets nothing else), so the probability is the default 0.99 whatever
    # the caller gives (resect passes 0.999)
    res, _, _, _ = abspose_images(bs, Xs, [0, len(np.asarray(bs).reshape(-1, 3))], threshold, iterations=iterations, probability=0.99,
                                  inlier_chord=0.0, ctx=ctx)
    return _invert_model(res[0]["lo_model"])


def reconstructed_points_for_images(tracks_manager, reconstruction, images: Iterable[str]) -> List[Tuple[str, int]]:
    """Number of reconstructed points visible on each image that is not in the reconstruction (``reconstruction.py:677-692``), sorted by
    decreasing count (a stable sort, the images in the order given)."""
    points = reconstruction.points
    res = {im: sum(1 for track in tracks_manager.get_shot_observations(im) if track in points)
           for im in images if im not in reconstruction.shots}
    return sorted(res.items(), key=lambda x: -x[1])


def _rig_assignments_per_image(rig_assignments) -> Dict[str, Tuple[str, str, List[str]]]:
    """``rig.rig_assignments_per_image``: image -> (instance id, rig camera id, the instance's images)"""
    per_image = {}
    for instance_id, instance in rig_assignments.items():
        instance_shots = [s[0] for s in instance]
        for shot_id, rig_camera_id in instance:
            per_image[shot_id] = (f"{instance_id}", rig_camera_id, instance_shots)
    return per_image


def _resect_rows(data, tracks_manager, reconstruction, shot_id: str):
    """the rows of resect's problem: (camera, normalised image points, point coordinates, track ids) of the image's reconstructed tracks"""
    camera = reconstruction.cameras[data.load_exif(shot_id)["camera"]]
    xy, Xs, ids = [], [], []
    for track, obs in tracks_manager.get_shot_observations(shot_id).items():
        if track in reconstruction.points:
            xy.append(obs.point)
            Xs.append(reconstruction.points[track].coordinates)
            ids.append(track)
    return camera, np.array(xy, np.float64).reshape(-1, 2), np.array(Xs, np.float64).reshape(-1, 3), ids


def _add_shot(data, reconstruction, rig_assignments, shot_id: str, pose, metadata_for: Optional[Callable]) -> Set[str]:
    """``add_shot`` (``reconstruction.py:247-285``); the shots' metadata comes from ``metadata_for(data, shot_id)`` when given"""
    from .geometry_types import Pose, RigInstance

    if shot_id not in rig_assignments:
        shot = reconstruction.create_shot(shot_id, data.load_exif(shot_id)["camera"], pose)
        if metadata_for is not None:
            shot.metadata = metadata_for(data, shot_id)
        return {shot_id}
    instance_id, _, instance_shots = rig_assignments[shot_id]
    rig_instance = reconstruction.add_rig_instance(RigInstance(instance_id))
    for shot in instance_shots:
        _, rig_camera_id, _ = rig_assignments[shot]
        created = reconstruction.create_shot(shot, data.load_exif(shot)["camera"], Pose(), rig_camera_id, instance_id)
        if metadata_for is not None:
            created.metadata = metadata_for(data, shot)
    rig_instance.update_instance_pose_with_shot(shot_id, pose)
    return set(instance_shots)


def _resect_finish(data, tracks_manager, reconstruction, rig_assignments, shot_id: str, ids: List[str], lo_model: np.ndarray,
                   inliers: np.ndarray, min_inliers: int, metadata_for: Optional[Callable], ctx) -> Tuple[bool, Set[str], Dict[str, Any]]:
    """resect after the estimator (``reconstruction.py:734-762``): the report, and on success the shot(s) and the inlier observations"""
    from .geometry_types import Pose

    ninliers = int(inliers.sum())
    report: Dict[str, Any] = {"num_common_points": len(ids), "num_inliers": ninliers}
    if ninliers < min_inliers:
        return False, set(), report
    T = _invert_model(lo_model)
    R = T[:, :3].T
    t = -R.dot(T[:, 3])
    assert shot_id not in reconstruction.shots
    pose = Pose(translation=t)  # pygeometry.Pose(R, t)
    pose.set_rotation_matrix(R)
    new_shots = _add_shot(data, reconstruction, rig_assignments, shot_id, pose, metadata_for)
    if shot_id in rig_assignments:
        triangulate_shot_features(tracks_manager, reconstruction, new_shots, data.config, ctx=ctx)
    for i in np.flatnonzero(inliers):
        reconstruction.add_observation(shot_id, ids[i], tracks_manager.get_observation(shot_id, ids[i]))
    report["shots"] = list(new_shots)
    return True, new_shots, report


def _resect_batch(data, tracks_manager, reconstruction, shot_ids: Sequence[str], threshold: float, ctx):
    """the estimator for several images against the reconstruction as it stands: per image (ids, lo_model or None below 5 rows, inlier mask)"""
    rows = [_resect_rows(data, tracks_manager, reconstruction, s) for s in shot_ids]
    solved = [k for k, r in enumerate(rows) if len(r[3]) >= 5]
    out: List[Tuple[List[str], Optional[np.ndarray], Optional[np.ndarray]]] = [(r[3], None, None) for r in rows]
    if not solved:
        return out
    cam_index: Dict[str, int] = {}
    models: List[int] = []
    params: List[np.ndarray] = []
    image_cam = []
    for k in solved:
        cam = rows[k][0]
        if cam.id not in cam_index:
            model, par = camera_parameters(cam)
            cam_index[cam.id] = len(models)
            models.append(model)
            params.append(par)
        image_cam.append(cam_index[cam.id])
    off = np.r_[0, np.cumsum([len(rows[k][3]) for k in solved])].astype(np.int64)
    # absolute_pose_ransac(bs, Xs, threshold, 1000, 0.999): the 0.999 is not passed on (multiview.py:475-476 sets only the iterations),
    # so the probability is the default 0.99
    res, _, cmask, _ = abspose_images_pixels(np.concatenate([rows[k][1] for k in solved]), np.concatenate([rows[k][2] for k in solved]), off,
                                             np.array(image_cam, np.int32), np.array(models, np.int32),
                                             np.array(params, np.float64).reshape(-1, 16), threshold, iterations=1000, probability=0.99,
                                             inlier_chord=threshold, ctx=ctx)
    for j, k in enumerate(solved):
        out[k] = (rows[k][3], res[j]["lo_model"], cmask[off[j]: off[j + 1]])
    return out


def resect(data, tracks_manager, reconstruction, shot_id: str, threshold: float, min_inliers: int, ctx=None,
           metadata_for: Optional[Callable] = None) -> Tuple[bool, Set[str], Dict[str, Any]]:
    """Try resecting and adding a shot to the reconstruction (``reconstruction.py:695-762``): same arguments, reports and map updates.
    The bearings, the LO-RANSAC and the inlier test run on the device.  ``metadata_for(data, shot_id)`` (optional) supplies the shots'
    metadata (the reference reads EXIF and the control plane there, ``helpers.get_image_metadata``); without it they keep the default."""
    rig_assignments = _rig_assignments_per_image(data.load_rig_assignments())
    ids, lo_model, inliers = _resect_batch(data, tracks_manager, reconstruction, [shot_id], threshold, ctx)[0]
    if lo_model is None:
        return False, set(), {"num_common_points": len(ids)}
    return _resect_finish(data, tracks_manager, reconstruction, rig_assignments, shot_id, ids, lo_model, inliers, min_inliers, metadata_for, ctx)


def resect_candidates(data, tracks_manager, reconstruction, candidates: Sequence[Tuple[str, int]], threshold: float, min_inliers: int,
                      max_batch: int = 8, ctx=None, metadata_for: Optional[Callable] = None) -> Dict[str, Any]:
    """The ``for image, _ in candidates`` loop of ``grow_reconstruction`` (``reconstruction.py:1525-1575``) up to its first success, as
    batched calls: the reconstruction does not change while candidates fail and every estimate seeds its own generator, so up to
    ``max_batch`` candidates are solved at once and the first that succeeds is taken -- the loop's result exactly.
    ``candidates``: what ``reconstructed_points_for_images`` returns.
    -> {"image": the image added or None, "new_shots": set, "report": its report or None, "failed": [(image, report), ...] of the
    candidates tried before it, in order}."""
    if max_batch < 1:
        raise ValueError("resect_candidates: max_batch must be at least 1")
    rig_assignments = _rig_assignments_per_image(data.load_rig_assignments())
    images = [c[0] for c in candidates]
    failed: List[Tuple[str, Dict[str, Any]]] = []
    for start in range(0, len(images), max_batch):
        batch = images[start: start + max_batch]
        for image, (ids, lo_model, inliers) in zip(batch, _resect_batch(data, tracks_manager, reconstruction, batch, threshold, ctx)):
            if lo_model is None:
                ok, new_shots, report = False, set(), {"num_common_points": len(ids)}
            else:
                ok, new_shots, report = _resect_finish(data, tracks_manager, reconstruction, rig_assignments, image, ids, lo_model, inliers,
                                                       min_inliers, metadata_for, ctx)
            if ok:
                return {"image": image, "new_shots": new_shots, "report": report, "failed": failed}
            failed.append((image, report))
    return {"image": None, "new_shots": set(), "report": None, "failed": failed}


# ------------------------------------------------------------------------------------------------
# bootstrap: the two-view 5-point reconstruction of candidate initial pairs (reconstruction.py:336-560)
# ------------------------------------------------------------------------------------------------
TWO_VIEW_STATUS = ("ok", "no configuration", "undecidable")


def _two_view_params(threshold: float, refine_iterations: int, check_reversal: bool, reversal_ratio: float, iterations: int, probability: float,
                     skip_inlier_tests: bool = False) -> TwoViewParams:
    return TwoViewParams(float(threshold), float(probability), float(reversal_ratio), int(iterations), 1, 10, int(refine_iterations),
                         int(bool(check_reversal)), int(bool(skip_inlier_tests)))


def _two_view_poses(poses, n_pairs: int, who: str):
    if poses is None:
        return None, C.POINTER(C.c_double)()
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    if len(poses) != n_pairs:
        raise ValueError(who + ": poses must be n_pairs x 12 (R row-major, then t)")
    return poses, _fptr(poses, C.c_double)


def _two_view_results(res, n_pairs: int) -> List[Dict[str, Any]]:
    out = []
    for p in range(n_pairs):
        r = res[p]
        out.append({"status": r.status, "chosen": r.chosen, "R": np.array(r.R).reshape(2, 3, 3), "t": np.array(r.t).reshape(2, 3),
                    "n_inliers": list(r.n_inliers), "refine_iterations": list(r.refine_iterations), "rotation": np.array(r.rotation),
                    "translation": np.array(r.translation), "lo_model": np.array(r.lo_model).reshape(3, 4), "score": r.score,
                    "iterations": r.iterations})
    return out


def two_view_pairs(b1: np.ndarray, b2: np.ndarray, offsets: Sequence[int], threshold: float, *, poses=None, refine_iterations: int = 1000,
                   check_reversal: bool = False, reversal_ratio: float = 1.0, iterations: int = 1000, probability: float = 0.99,
                   skip_inlier_tests: bool = False, ctx=None) -> Tuple[List[Dict[str, Any]], np.ndarray, float]:
    """``osfm_two_view_pairs``: the 5-point half of ``two_view_reconstruction_general`` for a batch of pairs on bearings (pair p owns rows
    offsets[p]:offsets[p+1] of b1 / b2), or, with `poses` (n_pairs x 12: R row-major, then t), ``two_view_reconstruction_5pt`` on given poses.
    -> (per-pair dicts: status (index into TWO_VIEW_STATUS), chosen (-1, 0, 1), R / t / n_inliers / refine_iterations per configuration,
    rotation / translation of the chosen one, the RANSAC's lo_model / score / iterations; mask (uint8 per row: bit 0 / 1 inlier of
    configuration 0 / 1, bit 2 of the chosen one); kernel milliseconds)."""
    ctx = ctx or default_context()
    b1 = np.ascontiguousarray(b1, np.float64).reshape(-1, 3)
    b2 = np.ascontiguousarray(b2, np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(offsets, np.int64)
    n_pairs = len(off) - 1
    if len(b1) != len(b2) or n_pairs < 0 or (n_pairs > 0 and off[-1] != len(b1)):
        raise ValueError("two_view_pairs: b1 / b2 / offsets do not agree")
    poses, poses_ptr = _two_view_poses(poses, n_pairs, "two_view_pairs")
    prm = _two_view_params(threshold, refine_iterations, check_reversal, reversal_ratio, iterations, probability, skip_inlier_tests)
    res = (TwoViewResult * max(n_pairs, 1))()
    mask = np.zeros(max(len(b1), 1), np.uint8)
    ms = C.c_double(0.0)
    check(load().osfm_two_view_pairs(ctx.handle, _fptr(b1, C.c_double), _fptr(b2, C.c_double), _fptr(off, C.c_int64), n_pairs, poses_ptr,
                                     C.byref(prm), res, _fptr(mask, C.c_uint8), C.byref(ms)), "osfm_two_view_pairs")
    return _two_view_results(res, n_pairs), mask[: len(b1)], ms.value


def two_view_pairs_pixels(p1: np.ndarray, p2: np.ndarray, offsets: Sequence[int], pair_cams: np.ndarray, cam_model: np.ndarray,
                          cam_params: np.ndarray, threshold: float, *, poses=None, refine_iterations: int = 1000, check_reversal: bool = False,
                          reversal_ratio: float = 1.0, iterations: int = 1000, probability: float = 0.99,
                          ctx=None) -> Tuple[List[Dict[str, Any]], np.ndarray, float]:
    """``osfm_two_view_pairs_pixels``: the same from normalised image coordinates, the bearings computed on the device with the cameras
    pair_cams[p] = (camera of side 1, camera of side 2) of the table cam_model (n_cams) / cam_params (n_cams x 16)."""
    ctx = ctx or default_context()
    p1 = np.ascontiguousarray(np.asarray(p1, np.float64).reshape(len(p1), -1)[:, :2])
    p2 = np.ascontiguousarray(np.asarray(p2, np.float64).reshape(len(p2), -1)[:, :2])
    off = np.ascontiguousarray(offsets, np.int64)
    n_pairs = len(off) - 1
    if len(p1) != len(p2) or n_pairs < 0 or (n_pairs > 0 and off[-1] != len(p1)):
        raise ValueError("two_view_pairs_pixels: p1 / p2 / offsets do not agree")
    pc = np.ascontiguousarray(pair_cams, np.int32)
    cm = np.ascontiguousarray(cam_model, np.int32)
    cp = np.ascontiguousarray(cam_params, np.float64)
    if pc.shape != (n_pairs, 2) or cm.ndim != 1 or cp.shape != (len(cm), 16):
        raise ValueError(f"two_view_pairs_pixels: pair_cams must be ({n_pairs}, 2) and cam_params ({len(cm)}, 16) for cam_model of length "
                         f"{len(cm)}; got {pc.shape}, {cp.shape}")
    poses, poses_ptr = _two_view_poses(poses, n_pairs, "two_view_pairs_pixels")
    prm = _two_view_params(threshold, refine_iterations, check_reversal, reversal_ratio, iterations, probability)
    res = (TwoViewResult * max(n_pairs, 1))()
    mask = np.zeros(max(len(p1), 1), np.uint8)
    ms = C.c_double(0.0)
    check(load().osfm_two_view_pairs_pixels(ctx.handle, _fptr(p1, C.c_double), _fptr(p2, C.c_double), _fptr(off, C.c_int64), n_pairs,
                                            _fptr(pc, C.c_int32), _fptr(cm, C.c_int32), _fptr(cp, C.c_double), len(cm), poses_ptr, C.byref(prm), res,
                                            _fptr(mask, C.c_uint8), C.byref(ms)), "osfm_two_view_pairs_pixels")
    return _two_view_results(res, n_pairs), mask[: len(p1)], ms.value


def _rotation_vector(R: np.ndarray) -> np.ndarray:
    """angle-axis of a rotation matrix through the quaternion, as the library's rotmat_to_aa (for a configuration that was not chosen)"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    q = np.zeros(4)
    trace = R[0, 0] + R[1, 1] + R[2, 2]
    if trace >= 0.0:
        s = np.sqrt(trace + 1.0)
        q[0] = 0.5 * s
        s = 0.5 / s
        q[1:] = [(R[2, 1] - R[1, 2]) * s, (R[0, 2] - R[2, 0]) * s, (R[1, 0] - R[0, 1]) * s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i + 1] = 0.5 * s
        s = 0.5 / s
        q[0] = (R[k, j] - R[j, k]) * s
        q[j + 1] = (R[j, i] + R[i, j]) * s
        q[k + 1] = (R[k, i] + R[i, k]) * s
    norm = float(np.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]))
    if norm > 0.0:
        two_theta = 2.0 * (np.arctan2(-norm, -q[0]) if q[0] < 0.0 else np.arctan2(norm, q[0]))
        return q[1:] * (two_theta / norm)
    return q[1:] * 2.0


def _triangulating_rows(b1: np.ndarray, b2: np.ndarray, R: np.ndarray, t: np.ndarray, threshold: float) -> np.ndarray:
    """the library's inlier test (inlier_bearing: the midpoint of the two rays, seen from both cameras within `threshold`) in numpy, for
    the handful of rows of a pair that is too small to reach the device -> indices"""
    b1 = np.asarray(b1, np.float64).reshape(-1, 3)
    b2 = np.asarray(b2, np.float64).reshape(-1, 3)
    keep = []
    for i, (x, y) in enumerate(zip(b1, b2)):
        ry = R.dot(y)
        a00, a10, a11 = x.dot(x), x.dot(ry), -ry.dot(ry)
        det = a00 * a11 + a10 * a10
        if -1e-10 < det < 1e-10:
            continue
        rhs0, rhs1 = t.dot(x), t.dot(ry)
        X = 0.5 * ((a11 * rhs0 + a10 * rhs1) / det * x + t + (-a10 * rhs0 + a00 * rhs1) / det * ry)
        q = R.T.dot(X - t)
        if np.linalg.norm(X / np.linalg.norm(X) - x) < threshold and np.linalg.norm(q / np.linalg.norm(q) - y) < threshold:
            keep.append(i)
    return np.array(keep, np.int64)


def two_view_reconstruction_and_refinement(b1: np.ndarray, b2: np.ndarray, R: np.ndarray, t: np.ndarray, threshold: float, iterations: int,
                                           transposed: bool, ctx=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Reconstruct two views using the provided rotation and translation (``reconstruction.py:336-374``): same arguments, same return
    (rotation vector, translation, inlier indices).  The rotation vector is the library's angle-axis of the matrix the reference hands to
    ``cv2.Rodrigues``."""
    pose = np.r_[np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]
    res, mask, _ = two_view_pairs(b1, b2, [0, len(b1)], threshold, poses=pose, refine_iterations=iterations, check_reversal=bool(transposed), ctx=ctx)
    c = 1 if transposed else 0
    if res[0]["n_inliers"][c] < 0:  # five or fewer correspondences: nothing ran, and nothing is refined in the reference either
        R0, t0 = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
        Rc, tc = (R0.T, -R0.T.dot(t0)) if transposed else (R0, t0)
        return _rotation_vector(Rc.T), -Rc.T.dot(tc), _triangulating_rows(b1, b2, Rc, tc, threshold)
    return _rotation_vector(res[0]["R"][c]), res[0]["t"][c].copy(), np.flatnonzero(mask >> c & 1)


def two_view_reconstruction_5pt(b1: np.ndarray, b2: np.ndarray, R: np.ndarray, t: np.ndarray, threshold: float, iterations: int,
                                check_reversal: bool = False, reversal_ratio: float = 1.0,
                                ctx=None) -> Tuple[Optional[np.ndarray], Optional[np.ndarray], Any]:
    """5-point reconstruction and refinement given the relative rotation and translation (``reconstruction.py:415-485``): same
    arguments, same return -- (rotation vector, translation, inlier indices), or (None, None, []) where no configuration has more than
    5 inliers or the two cannot be told apart."""
    pose = np.r_[np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]
    res, mask, _ = two_view_pairs(b1, b2, [0, len(b1)], threshold, poses=pose, refine_iterations=iterations, check_reversal=check_reversal,
                                  reversal_ratio=reversal_ratio, ctx=ctx)
    if res[0]["status"] != 0:
        return None, None, []
    return res[0]["rotation"], res[0]["translation"], np.flatnonzero(mask >> 2 & 1)


# ------------------------------------------------------------------------------------------------
# bootstrap: the plane-based two-view reconstruction (reconstruction.py:298-333, multiview.py:366-441)
# ------------------------------------------------------------------------------------------------
PLANE_STATUS = ("ok", "no homography", "degenerate homography")


def _plane_params(threshold: float, iterations: int, probability: float, use_lo: bool, lo_iterations: int,
                  use_iteration_reduction: bool) -> PlaneParams:
    return PlaneParams(float(threshold), float(probability), int(iterations), int(bool(use_lo)), int(lo_iterations),
                       int(bool(use_iteration_reduction)))


def _plane_results(res, n_pairs: int) -> List[Dict[str, Any]]:
    out = []
    for p in range(n_pairs):
        r = res[p]
        out.append({"status": r.status, "H": np.array(r.H).reshape(3, 3), "singular": np.array(r.singular), "h_inliers": r.h_inliers,
                    "iterations": r.iterations, "motion_inliers": list(r.motion_inliers), "chosen": r.chosen, "R": np.array(r.R).reshape(3, 3),
                    "t": np.array(r.t), "rotation": np.array(r.rotation), "translation": np.array(r.translation), "n_inliers": r.n_inliers})
    return out


def two_view_plane_pairs(b1: np.ndarray, b2: np.ndarray, offsets: Sequence[int], threshold: float, *, iterations: int = 1000,
                         probability: float = 0.99, use_lo: bool = True, lo_iterations: int = 10, use_iteration_reduction: bool = True,
                         ctx=None) -> Tuple[List[Dict[str, Any]], np.ndarray, float]:
    """``osfm_two_view_plane_pairs``: ``two_view_reconstruction_plane_based`` for a batch of pairs on bearings (pair p owns rows
    offsets[p]:offsets[p+1] of b1 / b2) -- a homography by LO-RANSAC, its eight motions, the one that explains the most rows.
    -> (per-pair dicts: status (index into PLANE_STATUS), H (middle singular value 1), singular, h_inliers, iterations, motion_inliers (8),
    chosen (-1 or 0 .. 7), R / t / rotation / translation / n_inliers of the chosen motion; mask (uint8 per row: bit 0 inlier of H, bit 1
    inlier of the chosen motion); kernel milliseconds)."""
    ctx = ctx or default_context()
    b1 = np.ascontiguousarray(b1, np.float64).reshape(-1, 3)
    b2 = np.ascontiguousarray(b2, np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(offsets, np.int64)
    n_pairs = len(off) - 1
    if len(b1) != len(b2) or n_pairs < 0 or (n_pairs > 0 and off[-1] != len(b1)):
        raise ValueError("two_view_plane_pairs: b1 / b2 / offsets do not agree")
    prm = _plane_params(threshold, iterations, probability, use_lo, lo_iterations, use_iteration_reduction)
    res = (PlaneResult * max(n_pairs, 1))()
    mask = np.zeros(max(len(b1), 1), np.uint8)
    ms = C.c_double(0.0)
    check(load().osfm_two_view_plane_pairs(ctx.handle, _fptr(b1, C.c_double), _fptr(b2, C.c_double), _fptr(off, C.c_int64), n_pairs, C.byref(prm),
                                           res, _fptr(mask, C.c_uint8), C.byref(ms)), "osfm_two_view_plane_pairs")
    return _plane_results(res, n_pairs), mask[: len(b1)], ms.value


def two_view_plane_pairs_pixels(p1: np.ndarray, p2: np.ndarray, offsets: Sequence[int], pair_cams: np.ndarray, cam_model: np.ndarray,
                                cam_params: np.ndarray, threshold: float, *, iterations: int = 1000, probability: float = 0.99,
                                use_lo: bool = True, lo_iterations: int = 10, use_iteration_reduction: bool = True,
                                ctx=None) -> Tuple[List[Dict[str, Any]], np.ndarray, float]:
    """``osfm_two_view_plane_pairs_pixels``: the same from normalised image coordinates, the bearings computed on the device with the
    cameras pair_cams[p] = (camera of side 1, camera of side 2) of the table cam_model (n_cams) / cam_params (n_cams x 16)."""
    ctx = ctx or default_context()
    p1 = np.ascontiguousarray(np.asarray(p1, np.float64).reshape(len(p1), -1)[:, :2])
    p2 = np.ascontiguousarray(np.asarray(p2, np.float64).reshape(len(p2), -1)[:, :2])
    off = np.ascontiguousarray(offsets, np.int64)
    n_pairs = len(off) - 1
    if len(p1) != len(p2) or n_pairs < 0 or (n_pairs > 0 and off[-1] != len(p1)):
        raise ValueError("two_view_plane_pairs_pixels: p1 / p2 / offsets do not agree")
    pc = np.ascontiguousarray(pair_cams, np.int32)
    cm = np.ascontiguousarray(cam_model, np.int32)
    cp = np.ascontiguousarray(cam_params, np.float64)
    if pc.shape != (n_pairs, 2) or cm.ndim != 1 or cp.shape != (len(cm), 16):
        raise ValueError(f"two_view_plane_pairs_pixels: pair_cams must be ({n_pairs}, 2) and cam_params ({len(cm)}, 16) for cam_model of length "
                         f"{len(cm)}; got {pc.shape}, {cp.shape}")
    prm = _plane_params(threshold, iterations, probability, use_lo, lo_iterations, use_iteration_reduction)
    res = (PlaneResult * max(n_pairs, 1))()
    mask = np.zeros(max(len(p1), 1), np.uint8)
    ms = C.c_double(0.0)
    check(load().osfm_two_view_plane_pairs_pixels(ctx.handle, _fptr(p1, C.c_double), _fptr(p2, C.c_double), _fptr(off, C.c_int64), n_pairs,
                                                  _fptr(pc, C.c_int32), _fptr(cm, C.c_int32), _fptr(cp, C.c_double), len(cm), C.byref(prm), res,
                                                  _fptr(mask, C.c_uint8), C.byref(ms)), "osfm_two_view_plane_pairs_pixels")
    return _plane_results(res, n_pairs), mask[: len(p1)], ms.value


def motion_from_plane_homography(H: np.ndarray, ctx=None) -> Optional[List[Tuple[np.ndarray, np.ndarray, np.ndarray, float]]]:
    """Candidate camera motions from a plane-induced homography (``multiview.py:366-441``): eight (R, t, n, d), or None where two singular
    values are nearly equal.  The signs of the singular vectors are fixed (plane_core.h), so the order is a property of H alone."""
    ctx = ctx or default_context()
    H = np.ascontiguousarray(H, np.float64).reshape(9)
    motions = np.zeros((8, 16))
    count = C.c_int(0)
    check(load().osfm_plane_motions(ctx.handle, _fptr(H, C.c_double), _fptr(motions, C.c_double), C.byref(count)), "osfm_plane_motions")
    if count.value == 0:
        return None
    return [(m[:9].reshape(3, 3).copy(), m[9:12].copy(), m[12:15].copy(), float(m[15])) for m in motions]


def two_view_reconstruction_plane_based(b1: np.ndarray, b2: np.ndarray, threshold: float,
                                        ctx=None) -> Tuple[Optional[np.ndarray], Optional[np.ndarray], Any]:
    """Reconstruct two views from point correspondences lying on a plane (``reconstruction.py:298-333``): same arguments, same return --
    (rotation vector, translation, inlier indices), or (None, None, []) without a homography or with a degenerate one.  The motion
    returned is the one with the most inliers (the reference's ``np.argmax`` over a map object always takes the first)."""
    res, mask, _ = two_view_plane_pairs(b1, b2, [0, len(b1)], threshold, ctx=ctx)
    if res[0]["status"] != 0:
        return None, None, []
    return res[0]["rotation"], res[0]["translation"], np.flatnonzero(mask >> 1 & 1)


def two_view_reconstruction_general_pairs(pairs: Sequence[Tuple[Any, Any, Any, Any]], threshold: float, iterations: int,
                                          check_reversal: bool = False, reversal_ratio: float = 1.0, *,
                                          plane_based=None, ctx=None) -> List[Tuple[Any, Any, Any, Dict[str, Any]]]:
    """``two_view_reconstruction_general`` (``reconstruction.py:488-560``) for a list of (p1, p2, camera1, camera2) in ONE GPU call: the
    bearings, the 5-point LO-RANSAC, both configurations and the choice.  -> [(R, t, inliers, report)] as the reference returns them.
    The plane-based branch: ``plane_based="device"`` runs it for the whole list in one more GPU call (``two_view_plane_pairs_pixels``);
    a callable ``plane_based(b1, b2, threshold) -> (R, t, inliers)`` supplies it per pair on the host (the reference's own
    ``two_view_reconstruction_plane_based`` fits); either is then compared as the reference compares.  Without the argument that branch
    counts as not valid with 0 inliers."""
    from . import matching

    if not pairs:
        return []
    cam_index: Dict[int, int] = {}
    models: List[int] = []
    params: List[np.ndarray] = []
    pair_cams = np.zeros((len(pairs), 2), np.int32)
    for k, (_, _, camera1, camera2) in enumerate(pairs):
        for side, cam in enumerate((camera1, camera2)):
            if id(cam) not in cam_index:
                model, par = camera_parameters(cam)
                cam_index[id(cam)] = len(models)
                models.append(model)
                params.append(par)
            pair_cams[k, side] = cam_index[id(cam)]
    p1 = np.concatenate([np.asarray(p[0], np.float64).reshape(len(p[0]), -1)[:, :2] for p in pairs])
    p2 = np.concatenate([np.asarray(p[1], np.float64).reshape(len(p[1]), -1)[:, :2] for p in pairs])
    off = np.r_[0, np.cumsum([len(p[0]) for p in pairs])].astype(np.int64)
    # relative_pose_ransac(b1, b2, threshold, 1000, 0.999): the 0.999 is not passed on (multiview.py:494-516 sets only the iterations),
    # so the probability is the default 0.99
    res, mask, _ = two_view_pairs_pixels(p1, p2, off, pair_cams, np.array(models, np.int32), np.array(params, np.float64).reshape(-1, 16), threshold,
                                         refine_iterations=iterations, check_reversal=check_reversal, reversal_ratio=reversal_ratio, iterations=1000,
                                         probability=0.99, ctx=ctx)
    if isinstance(plane_based, str):
        if plane_based != "device":
            raise ValueError('two_view_reconstruction_general_pairs: plane_based must be None, a callable or "device"')
        res_plane, mask_plane, _ = two_view_plane_pairs_pixels(p1, p2, off, pair_cams, np.array(models, np.int32),
                                                               np.array(params, np.float64).reshape(-1, 16), threshold, ctx=ctx)
    out = []
    for k, (q1, q2, camera1, camera2) in enumerate(pairs):
        valid_5pt = res[k]["status"] == 0
        inliers_5p = np.flatnonzero(mask[off[k]: off[k + 1]] >> 2 & 1) if valid_5pt else []
        R_plane, t_plane, inliers_plane = None, None, []
        if isinstance(plane_based, str):
            if res_plane[k]["status"] == 0:
                R_plane, t_plane = res_plane[k]["rotation"], res_plane[k]["translation"]
                inliers_plane = np.flatnonzero(mask_plane[off[k]: off[k + 1]] >> 1 & 1)
        elif plane_based is not None:
            R_plane, t_plane, inliers_plane = plane_based(matching.pixel_bearing_many(camera1, q1, ctx), matching.pixel_bearing_many(camera2, q2, ctx),
                                                          threshold)
        valid_plane = R_plane is not None and t_plane is not None
        report: Dict[str, Any] = {"5_point_inliers": len(inliers_5p), "plane_based_inliers": len(inliers_plane)}
        if valid_5pt and len(inliers_5p) > len(inliers_plane):
            report["method"] = "5_point"
            out.append((res[k]["rotation"], res[k]["translation"], inliers_5p, report))
        elif valid_plane:
            report["method"] = "plane_based"
            out.append((R_plane, t_plane, inliers_plane, report))
        else:
            report["decision"] = "Could not find initial motion"
            out.append((None, None, [], report))
    return out


def two_view_reconstruction_general(p1: np.ndarray, p2: np.ndarray, camera1, camera2, threshold: float, iterations: int,
                                    check_reversal: bool = False, reversal_ratio: float = 1.0, *, plane_based=None,
                                    ctx=None) -> Tuple[Any, Any, Any, Dict[str, Any]]:
    """Reconstruct two views from point correspondences (``reconstruction.py:488-560``): same arguments, same return
    (rotation vector, translation, inliers, report).  See two_view_reconstruction_general_pairs for `plane_based`."""
    return two_view_reconstruction_general_pairs([(p1, p2, camera1, camera2)], threshold, iterations, check_reversal, reversal_ratio,
                                                 plane_based=plane_based, ctx=ctx)[0]
