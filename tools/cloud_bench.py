"""Measurement of the two point-cloud filters of grow_reconstruction's tail (osfm_points_conditioning / osfm_points_isolation, cloud.hip)
on one MI355X.  Not part of bench.py's headline line.

Workload (defaults): synthetic.make_ba_scene(5000, 500000, 10) -- 5 000 shots, 500 000 points, 5 M observations, ground-truth poses and
points -- plus 1 % far points: 5 000 of the landmarks moved to uniform positions in a box three times the cloud's extent.

    python tools/cloud_bench.py [--shots 5000] [--points 500000] [--track 10] [--steps 3] [--cpu-points 20000] [--k 7]

Prints one JSON line: kernel milliseconds (HIP events) and end-to-end milliseconds of each library call (host counting sorts, uploads
and the sequential statistics included) on the whole workload.  The host baseline is the numpy restatement of tests/cloud_cases.py on one
thread.  Its isolation is all-pairs, so it cannot run on 500 000 points: under "prefix" the line holds both filters on the first
--cpu-points landmarks of the same scene (and their observations), the library's two calls and the restatement's two functions on
exactly that smaller workload, so that the two columns can be read side by side; nothing is extrapolated to the whole workload."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from opensfm_amd import opensfm_adapter, synthetic  # noqa: E402
from opensfm_amd._lib import default_context  # noqa: E402
from opensfm_amd.geometry_types import _rodrigues  # noqa: E402


def workload(shots: int, points: int, track: int, seed: int = 42):
    prob = synthetic.make_ba_scene(shots, points, track, seed=seed)
    rng = np.random.default_rng(seed)
    X = np.array(prob["gt_points"], np.float64)
    lo, hi = X.min(0), X.max(0)
    far = rng.choice(points, max(points // 100, 1), replace=False)
    X[far] = rng.uniform(lo - (hi - lo), hi + (hi - lo), (len(far), 3))
    pose = np.asarray(prob["gt_pose"], np.float64)  # camera-to-world angle-axis and origin (bundle::Pose)
    shot_pose = np.zeros((shots, 12))
    for s in range(shots):
        R = _rodrigues(-pose[s, :3])
        shot_pose[s, :9] = R.reshape(9)
        shot_pose[s, 9:] = -R @ pose[s, 3:]
    cam_params = np.zeros((1, 16))
    cam_params[0, :3] = [-0.1, 0.01, 0.7]
    return {"points": X, "shot_pose": shot_pose, "shot_camera": np.zeros(shots, np.int32), "cam_model": np.zeros(1, np.int32),
            "cam_params": cam_params, "obs_shot": np.asarray(prob["obs_shot"], np.int32), "obs_point": np.asarray(prob["obs_point"], np.int32)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=5000)
    ap.add_argument("--points", type=int, default=500000)
    ap.add_argument("--track", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--cpu-points", type=int, default=20000)
    ap.add_argument("--k", type=int, default=7)
    a = ap.parse_args()
    ctx = default_context()
    sc = workload(a.shots, a.points, a.track)
    args = (sc["points"], sc["shot_pose"], sc["shot_camera"], sc["cam_model"], sc["cam_params"], sc["obs_shot"], sc["obs_point"])
    opensfm_adapter.points_isolation(sc["points"][:4096], a.k, ctx=ctx)  # warm-up
    cond_k, cond_w, iso_k, iso_w = [], [], [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        cond = opensfm_adapter.points_conditioning(*args, ctx=ctx)
        cond_w.append(time.perf_counter() - t0)
        cond_k.append(cond["kernel_ms"])
        t0 = time.perf_counter()
        iso = opensfm_adapter.points_isolation(sc["points"], a.k, ctx=ctx)
        iso_w.append(time.perf_counter() - t0)
        iso_k.append(iso["kernel_ms"])
    out = {"workload": f"{a.shots} shots, {a.points} points, {len(sc['obs_shot'])} observations, 1 % far points, k = {a.k}",
           "conditioning_kernel_ms": float(np.median(cond_k)), "conditioning_wall_ms": 1e3 * float(np.median(cond_w)),
           "conditioning_removed": int(cond["removed"]), "conditioning_reasons": np.bincount(cond["reason"], minlength=6).tolist(),
           "isolation_kernel_ms": float(np.median(iso_k)), "isolation_wall_ms": 1e3 * float(np.median(iso_w)), "isolation_removed": int(iso["count"])}
    # the host: the numpy restatement (one thread) and the library on the same prefix of the scene
    import cloud_cases

    m = min(a.cpu_points, a.points)
    keep = sc["obs_point"] < m
    sub = dict(sc, points=sc["points"][:m], obs_shot=sc["obs_shot"][keep], obs_point=sc["obs_point"][keep])
    sub_args = (sub["points"], sub["shot_pose"], sub["shot_camera"], sub["cam_model"], sub["cam_params"], sub["obs_shot"], sub["obs_point"])
    prefix = {"landmarks": m, "observations": int(keep.sum())}
    t0 = time.perf_counter()
    cond = opensfm_adapter.points_conditioning(*sub_args, ctx=ctx)
    prefix["conditioning_wall_ms"], prefix["conditioning_kernel_ms"] = 1e3 * (time.perf_counter() - t0), cond["kernel_ms"]
    t0 = time.perf_counter()
    iso = opensfm_adapter.points_isolation(sub["points"], a.k, ctx=ctx)
    prefix["isolation_wall_ms"], prefix["isolation_kernel_ms"] = 1e3 * (time.perf_counter() - t0), iso["kernel_ms"]
    t0 = time.perf_counter()
    ref_cond = cloud_cases.conditioning_restatement(sub)
    prefix["conditioning_numpy_restatement_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    ref_iso = cloud_cases.isolation_restatement(sub["points"], a.k)
    prefix["isolation_numpy_restatement_ms"] = 1e3 * (time.perf_counter() - t0)
    prefix["conditioning_reasons_equal"] = bool(np.array_equal(cond["reason"], ref_cond["reason"]))
    prefix["isolation_bit_equal"] = bool(np.array_equal(iso["avg"], ref_iso["avg"]) and np.array_equal(iso["removed"], ref_iso["removed"]))
    out["prefix"] = prefix
    print(json.dumps(out))


if __name__ == "__main__":
    main()
