"""Measurement of the batched plane-based two-view reconstruction of bootstrap_reconstruction (osfm_two_view_plane_pairs, plane.hip) on
one MI355X.  Not part of bench.py's headline line.

Workload (defaults): 2 000 pairs, N uniform in [50, 2000] correspondences (the size mix of tools/twoview_bench.py), here planar scenes
(tests/plane_cases.py) with 30 % gross outliers and noise of a tenth of the threshold; threshold 0.004, 1000 iterations, probability
0.99, LO on.

    python tools/plane_bench.py [--pairs 2000] [--nmin 50] [--nmax 2000] [--steps 7] [--general-pairs 200]

The calls alternate within one process, `steps` times each, and every figure is reported as median [min, max]:
  plane                osfm_two_view_plane_pairs on the bearings: kernel ms (HIP events) and end-to-end wall ms of the Python call
  plane_pixels         osfm_two_view_plane_pairs_pixels on normalised image coordinates (the bearings on the device)
  five_point_pixels    two_view_pairs_pixels on the same batch: the 5-point call the plane call runs beside
  general / general_device   two_view_reconstruction_general_pairs over the first `general-pairs` pairs without / with
                       plane_based="device" (wall ms: the Python loop over the pairs is part of it), and how the reports divide."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from opensfm_amd import matching, reconstruction  # noqa: E402
from opensfm_amd._lib import default_context  # noqa: E402

THRESHOLD = 0.004


def workload(pairs: int, nmin: int, nmax: int, seed: int = 1):
    import plane_cases as cases

    rng = np.random.default_rng(seed)
    parts = [cases.plane_scene(rng, int(rng.integers(nmin, nmax + 1)), outliers=0.3, noise=THRESHOLD / 10) for _ in range(pairs)]
    b1 = np.concatenate([p[0] for p in parts])
    b2 = np.concatenate([p[1] for p in parts])
    off = np.r_[0, np.cumsum([len(p[0]) for p in parts])].astype(np.int64)
    planted = np.array([len(p[2]) for p in parts])
    return b1, b2, off, planted


def stats(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--nmin", type=int, default=50)
    ap.add_argument("--nmax", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--general-pairs", type=int, default=200)
    a = ap.parse_args()
    ctx = default_context()
    b1, b2, off, planted = workload(a.pairs, a.nmin, a.nmax)
    # an undistorted perspective camera of focal 1: the normalised image coordinates are the euclidean ones
    cam = types.SimpleNamespace(projection_type="perspective", focal=1.0, k1=0.0, k2=0.0)
    p1, p2 = b1[:, :2] / b1[:, 2:3], b2[:, :2] / b2[:, 2:3]
    model, par = matching.camera_parameters(cam)
    table = (np.zeros((a.pairs, 2), np.int32), np.array([model], np.int32), np.array([par], np.float64).reshape(1, 16))
    g = min(a.general_pairs, a.pairs)
    general = [(p1[off[k]: off[k + 1]], p2[off[k]: off[k + 1]], cam, cam) for k in range(g)]
    calls = {
        "plane": lambda: reconstruction.two_view_plane_pairs(b1, b2, off, THRESHOLD, ctx=ctx),
        "plane_pixels": lambda: reconstruction.two_view_plane_pairs_pixels(p1, p2, off, *table, THRESHOLD, ctx=ctx),
        "five_point_pixels": lambda: reconstruction.two_view_pairs_pixels(p1, p2, off, *table, THRESHOLD, ctx=ctx),
        "general": lambda: (reconstruction.two_view_reconstruction_general_pairs(general, THRESHOLD, 1000, ctx=ctx), None, float("nan")),
        "general_device": lambda: (reconstruction.two_view_reconstruction_general_pairs(general, THRESHOLD, 1000, plane_based="device", ctx=ctx), None,
                                   float("nan")),
    }
    last = {}
    for name, call in calls.items():  # warm-up of every shape the timed window uses
        last[name] = call()
    kernel_ms = {k: [] for k in calls}
    wall_ms = {k: [] for k in calls}
    for step in range(a.steps):
        print("step %d of %d" % (step + 1, a.steps), file=sys.stderr, flush=True)
        for name, call in calls.items():
            t0 = time.perf_counter()
            out = call()
            wall_ms[name].append(1e3 * (time.perf_counter() - t0))
            kernel_ms[name].append(out[2])
    out = {"workload": f"{a.pairs} planar pairs, N in [{a.nmin}, {a.nmax}] ({int(off[-1])} correspondences), 30 % outliers", "steps": a.steps}
    for name in calls:
        out[name] = {"wall_ms": stats(wall_ms[name])}
        if not name.startswith("general"):
            out[name]["kernel_ms"] = stats(kernel_ms[name])
    res = last["plane"][0]
    status = np.array([r["status"] for r in res])
    out["plane"]["status_counts"] = {s: int((status == k).sum()) for k, s in enumerate(reconstruction.PLANE_STATUS)}
    out["plane"]["pairs_with_exactly_the_planted_h_inliers"] = int(sum(r["h_inliers"] == n for r, n in zip(res, planted)))
    out["plane"]["mean_iterations"] = float(np.mean([r["iterations"] for r in res]))
    out["plane"]["pairs_per_s_end_to_end"] = a.pairs / (out["plane"]["wall_ms"]["median"] / 1e3)
    for name in ("general", "general_device"):
        methods = [r[3].get("method", "none") for r in last[name][0]]
        out[name]["pairs"] = g
        out[name]["methods"] = {m: methods.count(m) for m in sorted(set(methods))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
