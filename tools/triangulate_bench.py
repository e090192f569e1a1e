"""Measurement of the track triangulation (osfm_triangulate_tracks, triangulate.hip) on one MI355X.  Not part of bench.py's headline line.

Workload (defaults): synthetic.make_ba_scene(5000, 500000, 10) -- 5 000 shots, 500 000 tracks, 5 M observations with pixel noise and
5 % gross mismatches -- with the ground-truth poses perturbed (1e-3 rad, 5 mm) so that the midpoint is not the answer and the refinement
has work to do.  ``--ragged`` takes the scene's ragged tracks instead (lengths 2 + Poisson(8), 15 % of the sightings missing), which
puts tracks on both kernels.

    python tools/triangulate_bench.py [--shots 5000] [--tracks 500000] [--track 10] [--ragged] [--steps 5] [--small 3000] [--no-host] [--robust]

Prints one JSON line.  "retriangulate": the whole workload in one call, as reconstruction.retriangulate issues it -- kernel milliseconds
(HIP events), end-to-end milliseconds of the array call (uploads and downloads included), tracks per second of kernel time, and the
fraction of the HBM bound the kernel time amounts to (20 B read per observation, 32 B written per track, at --hbm-tbs).  "shot_features":
the first --small tracks, the size of a triangulate_shot_features call after one resected image.  "host": the same --small call through
the HOST BUILD of triangulate.hip (tests/native/build_triangulate_emu.py: the same kernels on one CPU thread, lanes as fibres -- an
emulation made for testing, not an optimised CPU implementation), with whether its results equal the GPU's.
``--robust`` adds "robust": the same two calls through osfm_triangulate_tracks_robust (`triangulation_type: ROBUST`, the library's
generator with --seed) beside the FULL figures of the same build and scene, with the mean tries_used and inlier share, so that the
cost per try can be read off."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from opensfm_amd import _lib, reconstruction, synthetic  # noqa: E402
from opensfm_amd.geometry_types import _rodrigues  # noqa: E402


def workload(shots: int, tracks: int, track: int, ragged: bool, seed: int = 42):
    prob = synthetic.make_ba_scene(shots, tracks, track, seed=seed, ragged=ragged)
    rng = np.random.default_rng(seed + 1)
    pose = np.asarray(prob["gt_pose"], np.float64).copy()  # camera-to-world angle-axis and origin (bundle::Pose)
    pose[:, :3] += rng.normal(0, 1e-3, (shots, 3))
    pose[:, 3:] += rng.normal(0, 5e-3, (shots, 3))
    shot_pose = np.zeros((shots, 12))
    for s in range(shots):
        R = _rodrigues(-pose[s, :3])
        shot_pose[s, :9] = R.reshape(9)
        shot_pose[s, 9:] = -R @ pose[s, 3:]
    order = np.argsort(prob["obs_point"], kind="stable")  # track-major, shots ascending inside a track
    cam_params = np.zeros((1, 16))
    cam_params[0, :3] = [-0.1, 0.01, 0.7]
    counts = np.bincount(prob["obs_point"], minlength=tracks)
    return {"shot_pose": shot_pose, "shot_camera": np.zeros(shots, np.int32), "cam_model": np.zeros(1, np.int32), "cam_params": cam_params,
            "obs_shot": np.ascontiguousarray(prob["obs_shot"][order], np.int32), "obs_xy": np.ascontiguousarray(prob["obs_xy"][order], np.float64),
            "offsets": np.r_[0, np.cumsum(counts)].astype(np.int64)}


def prefix(sc, n_tracks):
    end = int(sc["offsets"][n_tracks])
    return dict(sc, obs_shot=sc["obs_shot"][:end], obs_xy=sc["obs_xy"][:end], offsets=sc["offsets"][:n_tracks + 1])


def call(sc, ctx=None):
    t0 = time.perf_counter()
    out = reconstruction.triangulate_tracks_arrays(sc["shot_pose"], sc["shot_camera"], sc["cam_model"], sc["cam_params"], sc["obs_shot"], sc["obs_xy"],
                                                   sc["offsets"], ctx=ctx)
    return out, 1e3 * (time.perf_counter() - t0)


def call_robust(sc, seed, ctx=None):
    t0 = time.perf_counter()
    out = reconstruction.triangulate_tracks_arrays_robust(sc["shot_pose"], sc["shot_camera"], sc["cam_model"], sc["cam_params"], sc["obs_shot"],
                                                          sc["obs_xy"], sc["offsets"], seed=seed, ctx=ctx)
    return out, 1e3 * (time.perf_counter() - t0)


def measure_robust(sc, steps, seed, ctx):
    kernel, wall = [], []
    for _ in range(steps):
        out, ms = call_robust(sc, seed, ctx)
        kernel.append(out[5])
        wall.append(ms)
    n_tracks, n_obs = len(sc["offsets"]) - 1, len(sc["obs_shot"])
    k = float(np.median(kernel))
    tries = float(out[4].sum())
    return out, {"tracks": n_tracks, "observations": n_obs, "kernel_ms": k, "kernel_ms_min": float(np.min(kernel)), "wall_ms": float(np.median(wall)),
                 "tracks_per_s": n_tracks / (k * 1e-3), "status_counts": np.bincount(out[1], minlength=7).tolist(),
                 "mean_tries_used": tries / max(n_tracks, 1), "kernel_us_per_1000_tries": 1e6 * k / max(tries, 1.0),
                 "inlier_share_of_triangulated": float(out[3].sum()) / max(float(np.diff(sc["offsets"])[out[1] == 0].sum()), 1.0)}


def measure(sc, steps, hbm_tbs, ctx):
    kernel, wall = [], []
    for _ in range(steps):
        out, ms = call(sc, ctx)
        kernel.append(out[3])
        wall.append(ms)
    n_tracks, n_obs = len(sc["offsets"]) - 1, len(sc["obs_shot"])
    k = float(np.median(kernel))
    bound_ms = (20.0 * n_obs + 32.0 * n_tracks) / (hbm_tbs * 1e12) * 1e3
    lengths = np.diff(sc["offsets"])
    return out, {"tracks": n_tracks, "observations": n_obs, "longest_track": int(lengths.max()), "median_track": float(np.median(lengths)),
                 "kernel_ms": k, "kernel_ms_min": float(np.min(kernel)), "wall_ms": float(np.median(wall)), "tracks_per_s": n_tracks / (k * 1e-3),
                 "hbm_bound_ms": bound_ms, "fraction_of_hbm_bound": bound_ms / k, "status_counts": np.bincount(out[1], minlength=6).tolist(),
                 "iteration_counts": np.bincount(out[2]).tolist()}


def host_build(sc, gpu_out):
    """the same call through the host emulation of triangulate.hip"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_triangulate_emu", os.path.join(ROOT, "tests", "native", "build_triangulate_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = C.CDLL(mod.build())
    for name, (res, args) in _lib._signatures().items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    old_lib, old_ctx = _lib._lib, getattr(_lib._tls, "ctx", None)
    _lib._lib, _lib._tls.ctx = lib, {}
    try:
        call(prefix(sc, min(64, len(sc["offsets"]) - 1)))  # warm-up (the fibres' stacks)
        out, ms = call(sc)
    finally:
        for c in _lib._tls.ctx.values():
            c.close()
        _lib._lib, _lib._tls.ctx = old_lib, old_ctx
    n_tracks = len(sc["offsets"]) - 1
    ok = ~np.isnan(gpu_out[0]).any(axis=1)
    diff = float((np.linalg.norm(out[0][ok] - gpu_out[0][ok], axis=1) / np.linalg.norm(gpu_out[0][ok], axis=1)).max()) if ok.any() else 0.0
    return {"tracks": n_tracks, "wall_ms": ms, "tracks_per_s": n_tracks / (ms * 1e-3),
            "statuses_and_iterations_equal_gpu": bool(np.array_equal(out[1], gpu_out[1]) and np.array_equal(out[2], gpu_out[2])),
            "largest_relative_point_difference_to_gpu": diff}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=5000)
    ap.add_argument("--tracks", type=int, default=500000)
    ap.add_argument("--track", type=int, default=10)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--small", type=int, default=3000)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth the bound is computed with, TB/s (MI355X: 8)")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--robust", action="store_true", help="also measure osfm_triangulate_tracks_robust on the same scene")
    ap.add_argument("--seed", type=int, default=0, help="seed of the robust call's generator")
    a = ap.parse_args()
    ctx = _lib.default_context()
    sc = workload(a.shots, a.tracks, a.track, a.ragged)
    small = prefix(sc, min(a.small, a.tracks))
    call(small, ctx)  # warm-up
    call(sc, ctx)     # ... and the context's block cache at full size
    out = {"workload": f"{a.shots} shots, {a.tracks} tracks, {len(sc['obs_shot'])} observations" + (", ragged" if a.ragged else ""),
           "library": os.path.basename(_lib.LIB_PATH)}
    _, out["retriangulate"] = measure(sc, a.steps, a.hbm_tbs, ctx)
    small_out, out["shot_features"] = measure(small, a.steps, a.hbm_tbs, ctx)
    again, _ = call(small, ctx)
    out["two_runs_bit_equal"] = bool(all(x.tobytes() == y.tobytes() for x, y in zip(again[:3], small_out[:3])))
    if a.robust:
        call_robust(small, a.seed, ctx)  # warm-up
        call_robust(sc, a.seed, ctx)
        out["robust"] = {}
        _, out["robust"]["retriangulate"] = measure_robust(sc, a.steps, a.seed, ctx)
        first, out["robust"]["shot_features"] = measure_robust(small, a.steps, a.seed, ctx)
        again, _ = call_robust(small, a.seed, ctx)
        out["robust"]["two_runs_bit_equal"] = bool(all(x.tobytes() == y.tobytes() for x, y in zip(again[:5], first[:5])))
    if not a.no_host:
        out["host"] = host_build(small, small_out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
