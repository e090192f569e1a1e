"""Raw depthmaps, their cleaning, pruning and merging on the GPU (``opensfm/dense.py`` compute_depthmap / clean_depthmap / prune_depthmap /
merge_depthmaps, ``dense::DepthmapEstimator``, ``dense::DepthmapCleaner`` and ``dense::DepthmapPruner``) for a batch of shots in one call
of ``osfm_depthmap_estimate`` / ``osfm_depthmap_clean`` / ``osfm_depthmap_prune``.

A problem of the estimator is ``{"views": [(K, R, t, image, mask), ...], "min_depth": float, "max_depth": float}`` with the shot itself
first, as ``add_views_to_depth_estimator`` adds them; of the cleaner ``{"views": [(K, R, t, depth), ...]}``; of the pruner
``{"views": [(K, R, t, depth, plane, color, label), ...]}``.  K, R are 3 x 3, t has 3 entries; images, masks and labels are uint8
(height, width), depths float32, planes float32 (height, width, 3), colors uint8 (height, width, 3).  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

METHODS = {"BRUTE_FORCE": 0, "PATCH_MATCH": 1, "PATCH_MATCH_SAMPLE": 2}
QUANTILES, PERTURBATIONS, WEIGHT_R2 = 4096, 6, 99
DEFAULT_SEED = 0x5EED


def default_params() -> _lib.DepthmapParams:
    p = _lib.DepthmapParams()
    _lib.load().osfm_depthmap_params_default(C.byref(p))
    return p


def params_from_config(config: Optional[dict] = None, **override) -> _lib.DepthmapParams:
    """``osfm_depthmap_params`` from the ``depthmap_*`` keys of an OpenSfM config (missing keys: the defaults of config.py)"""
    p = default_params()
    config = config or {}
    for field, key in (("min_depth", "depthmap_min_depth"), ("max_depth", "depthmap_max_depth"), ("min_patch_sd", "depthmap_min_patch_sd"),
                       ("min_correlation_score", "depthmap_min_correlation_score"), ("same_depth_threshold", "depthmap_same_depth_threshold"),
                       ("resolution", "depthmap_resolution"), ("num_neighbors", "depthmap_num_neighbors"),
                       ("num_matching_views", "depthmap_num_matching_views"), ("patchmatch_iterations", "depthmap_patchmatch_iterations"),
                       ("patch_size", "depthmap_patch_size"), ("min_consistent_views", "depthmap_min_consistent_views")):
        if key in config:
            setattr(p, field, config[key])
    if "depthmap_method" in config:
        method = config["depthmap_method"]
        if method not in METHODS:
            raise ValueError("Unknown depthmap method type (must be BRUTE_FORCE, PATCH_MATCH or PATCH_MATCH_SAMPLE)")
        p.method = METHODS[method]
    for field, value in override.items():
        setattr(p, field, value)
    return p


def tables(min_depth: Optional[float] = None, max_depth: Optional[float] = None) -> Dict[str, np.ndarray]:
    """the tables the library uses (``osfm_depthmap_tables``): normal, factor, weight and, for a depth range, init_depth"""
    out = {"normal": np.empty(QUANTILES, np.float32), "factor": np.empty((PERTURBATIONS, QUANTILES), np.float32),
           "weight": np.empty((256, WEIGHT_R2), np.float32)}
    init = None
    if min_depth is not None:
        out["init_depth"] = np.empty(QUANTILES, np.float32)
        init = out["init_depth"].ctypes.data_as(C.POINTER(C.c_float))
    ptr = [out[k].ctypes.data_as(C.POINTER(C.c_float)) for k in ("normal", "factor", "weight")]
    _lib.check(_lib.load().osfm_depthmap_tables(float(min_depth or 0.0), float(max_depth or 0.0), ptr[0], ptr[1], ptr[2], init), "osfm_depthmap_tables")
    return out


def _pointers(arrays: Sequence[Optional[np.ndarray]]):
    return (C.c_void_p * max(len(arrays), 1))(*[None if a is None or a.size == 0 else a.ctypes.data for a in arrays])


def _pack_views(problems, data_dtype, n_data: int):
    """offsets, K, R, t, per-view arrays and sizes of a batch; the arrays returned are kept alive by the caller"""
    offsets = np.zeros(len(problems) + 1, np.int32)
    K, R, t, data, widths, heights = [], [], [], [[] for _ in range(n_data)], [], []
    for b, problem in enumerate(problems):
        views = problem["views"]
        offsets[b + 1] = offsets[b] + len(views)
        for view in views:
            K.append(np.asarray(view[0], np.float64).reshape(9))
            R.append(np.asarray(view[1], np.float64).reshape(9))
            t.append(np.asarray(view[2], np.float64).reshape(3))
            first = np.ascontiguousarray(view[3], data_dtype)
            if first.ndim != 2:
                raise ValueError("a view's image / depth must be a (height, width) array")
            for k in range(n_data):
                a = np.ascontiguousarray(view[3 + k], data_dtype)
                if a.shape != first.shape:
                    raise ValueError("image and mask must have matching shapes.")
                data[k].append(a)
            heights.append(first.shape[0])
            widths.append(first.shape[1])
    flat = [np.ascontiguousarray(np.concatenate(x) if x else np.zeros(0), np.float64) for x in (K, R, t)]
    return offsets, flat, data, np.asarray(widths, np.int32), np.asarray(heights, np.int32)


def _dptr(a: np.ndarray, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def estimate_raw(problems: Sequence[dict], params: _lib.DepthmapParams, seed: int = DEFAULT_SEED,
                 device: Optional[int] = None) -> Tuple[List[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]], float]:
    """``osfm_depthmap_estimate``: per problem (depth, plane, score, nghbr) exactly as the estimator returns them, and the kernel ms"""
    offsets, (K, R, t), (images, masks), widths, heights = _pack_views(problems, np.uint8, 2)
    outs = []
    for b, problem in enumerate(problems):
        h, w = (images[offsets[b]].shape if len(problem["views"]) else (0, 0))
        outs.append((np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w), np.int32)))
    lo = np.asarray([float(p.get("min_depth", params.min_depth)) for p in problems], np.float64)
    hi = np.asarray([float(p.get("max_depth", params.max_depth)) for p in problems], np.float64)
    ms = C.c_double(0.0)
    ctx = _lib.default_context(device)
    _lib.check(_lib.load().osfm_depthmap_estimate(
        ctx.handle, len(problems), _dptr(offsets, C.c_int32), _dptr(K, C.c_double), _dptr(R, C.c_double), _dptr(t, C.c_double),
        _pointers(images), _pointers(masks), _dptr(widths, C.c_int32), _dptr(heights, C.c_int32), _dptr(lo, C.c_double), _dptr(hi, C.c_double),
        C.byref(params), C.c_uint64(int(seed) & (2 ** 64 - 1)), _pointers([o[0] for o in outs]), _pointers([o[1] for o in outs]),
        _pointers([o[2] for o in outs]), _pointers([o[3] for o in outs]), C.byref(ms)), "osfm_depthmap_estimate")
    return outs, ms.value


def clean_raw(problems: Sequence[dict], params: _lib.DepthmapParams, device: Optional[int] = None) -> Tuple[List[np.ndarray], float]:
    """``osfm_depthmap_clean``: per problem the cleaned depthmap of its first view, and the kernel ms"""
    offsets, (K, R, t), (depths,), widths, heights = _pack_views(problems, np.float32, 1)
    outs = [np.zeros(depths[offsets[b]].shape if len(problem["views"]) else (0, 0), np.float32) for b, problem in enumerate(problems)]
    ms = C.c_double(0.0)
    ctx = _lib.default_context(device)
    _lib.check(_lib.load().osfm_depthmap_clean(
        ctx.handle, len(problems), _dptr(offsets, C.c_int32), _dptr(K, C.c_double), _dptr(R, C.c_double), _dptr(t, C.c_double), _pointers(depths),
        _dptr(widths, C.c_int32), _dptr(heights, C.c_int32), C.byref(params), _pointers(outs), C.byref(ms)), "osfm_depthmap_clean")
    return outs, ms.value


def compute_depthmaps_arrays(problems: Sequence[dict], config: Optional[dict] = None, seed: int = DEFAULT_SEED, device: Optional[int] = None):
    """``dense.compute_depthmap`` for every problem: per problem (depth, plane, score, nghbr) with
    ``depth * (depth < max_depth) * (score > depthmap_min_correlation_score)`` applied, as the reference does before it saves"""
    params = params_from_config(config)
    raw, _ = estimate_raw(problems, params, seed, device)
    done = []
    for problem, (depth, plane, score, nghbr) in zip(problems, raw):
        good_score = score > params.min_correlation_score
        depth = depth * (depth < float(problem.get("max_depth", params.max_depth))) * good_score
        done.append((depth, plane, score, nghbr))
    return done


def clean_depthmaps_arrays(problems: Sequence[dict], config: Optional[dict] = None, device: Optional[int] = None) -> List[np.ndarray]:
    """``dense.clean_depthmap`` for every problem"""
    return clean_raw(problems, params_from_config(config), device)[0]


def _pack_prune_views(problems):
    """``_pack_views`` for the pruner's four arrays per view (two dtypes, two of them with three channels); the messages are the
    wrapper's (depthmap_bind.h:113-124)"""
    offsets = np.zeros(len(problems) + 1, np.int32)
    K, R, t, data, widths, heights = [], [], [], [[], [], [], []], [], []
    for b, problem in enumerate(problems):
        views = problem["views"]
        offsets[b + 1] = offsets[b] + len(views)
        for view in views:
            K.append(np.asarray(view[0], np.float64).reshape(9))
            R.append(np.asarray(view[1], np.float64).reshape(9))
            t.append(np.asarray(view[2], np.float64).reshape(3))
            depth, plane = np.ascontiguousarray(view[3], np.float32), np.ascontiguousarray(view[4], np.float32)
            color, label = np.ascontiguousarray(view[5], np.uint8), np.ascontiguousarray(view[6], np.uint8)
            if depth.ndim != 2:
                raise ValueError("a view's depth must be a (height, width) array")
            for name, a, channels in (("plane", plane, 3), ("color", color, 3), ("label", label, 0)):
                if a.shape[:2] != depth.shape:
                    raise ValueError(f"depth and {name} must have matching shapes.")
                if a.shape[2:] != ((channels,) if channels else ()):
                    raise ValueError(f"a view's {name} must be a (height, width" + (f", {channels})" if channels else ")") + " array")
            for k, a in enumerate((depth, plane, color, label)):
                data[k].append(a)
            heights.append(depth.shape[0])
            widths.append(depth.shape[1])
    flat = [np.ascontiguousarray(np.concatenate(x) if x else np.zeros(0), np.float64) for x in (K, R, t)]
    return offsets, flat, data, np.asarray(widths, np.int32), np.asarray(heights, np.int32)


Cloud = Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]


def prune_raw(problems: Sequence[dict], params: _lib.DepthmapParams, device: Optional[int] = None) -> Tuple[Cloud, np.ndarray, float]:
    """``osfm_depthmap_prune``: the merged cloud of the batch -- points (n, 3) float32, normals (n, 3) float32, colors (n, 3) uint8,
    labels (n,) uint8, the rows of problem 0 first --, the rows of every problem and the kernel ms"""
    offsets, (K, R, t), (depths, planes, colors, labels), widths, heights = _pack_prune_views(problems)
    first = [depths[offsets[b]] for b, problem in enumerate(problems) if len(problem["views"])]
    capacity = int(sum(np.count_nonzero(~(d <= 0)) for d in first))  # depth > 0 or NaN: the pixels Prune does not skip
    points, normals = np.empty((capacity, 3), np.float32), np.empty((capacity, 3), np.float32)
    out_colors, out_labels = np.empty((capacity, 3), np.uint8), np.empty(capacity, np.uint8)
    counts = np.zeros(len(problems), np.int64)
    ms = C.c_double(0.0)
    ctx = _lib.default_context(device)
    _lib.check(_lib.load().osfm_depthmap_prune(
        ctx.handle, len(problems), _dptr(offsets, C.c_int32), _dptr(K, C.c_double), _dptr(R, C.c_double), _dptr(t, C.c_double), _pointers(depths),
        _pointers(planes), _pointers(colors), _pointers(labels), _dptr(widths, C.c_int32), _dptr(heights, C.c_int32), C.byref(params),
        C.c_int64(capacity), _dptr(points, C.c_float), _dptr(normals, C.c_float), _dptr(out_colors, C.c_uint8), _dptr(out_labels, C.c_uint8),
        _dptr(counts, C.c_int64), C.byref(ms)), "osfm_depthmap_prune")
    n = int(counts.sum())
    return (points[:n], normals[:n], out_colors[:n], out_labels[:n]), counts, ms.value


def prune_depthmaps_arrays(problems: Sequence[dict], config: Optional[dict] = None, device: Optional[int] = None) -> List[Cloud]:
    """``dense.prune_depthmap`` for every problem: per problem (points, normals, colors, labels), views into the merged buffers"""
    merged, counts, _ = prune_raw(problems, params_from_config(config), device)
    ends = np.cumsum(counts)
    return [tuple(a[e - c:e] for a in merged) for c, e in zip(counts, ends)]


def merge_depthmaps_arrays(problems: Sequence[dict], config: Optional[dict] = None, device: Optional[int] = None) -> Cloud:
    """``dense.prune_depthmap`` for every problem and ``dense.merge_depthmaps`` of the results: the four concatenated arrays (no
    problems: four empty arrays, as ``merge_depthmaps_from_provider`` returns)"""
    if not len(problems):
        return np.array([]), np.array([]), np.array([]), np.array([])
    return prune_raw(problems, params_from_config(config), device)[0]
