"""Measurement of the batched two-view 5-point reconstruction of bootstrap_reconstruction (osfm_two_view_pairs, twoview.hip) on one
MI355X.  Not part of bench.py's headline line.

Workload (defaults): 2 000 pairs, N uniform in [50, 2000] correspondences (the size mix of tools/relrot_bench.py), mismatch fractions
uniform in [0, 0.6], noise 1e-3; threshold 0.004, 1000 RANSAC iterations, probability 0.99, LO on, five_point_refine_rec_iterations 1000.

    python tools/twoview_bench.py [--pairs 2000] [--nmin 50] [--nmax 2000] [--steps 7] [--cpu-pairs 48]

The calls alternate within one process, `steps` times each, and every figure is reported as median [min, max]:
  ransac_alone         matching.relpose_pairs(mode="ransac") on the batch: the rounds of the LO-RANSAC on their own (the baseline the
                       finish is added to)
  two_view / two_view_reversal      osfm_two_view_pairs with the RANSAC first, without / with check_reversal: kernel ms (HIP events)
                       and end-to-end wall ms of the Python call
  finish / finish_reversal          the same on given poses (the RANSAC's, inverted): tv_config_kernel + tv_decide_kernel alone
and the mean TinySolver iterations per configuration.  The host build of the same header (tests/native/twoview_host.cpp) runs a sample of
the same pairs on ONE thread, RANSAC included, for the second baseline."""
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
from opensfm_amd import matching, reconstruction  # noqa: E402
from opensfm_amd._lib import default_context  # noqa: E402

THRESHOLD = 0.004


def workload(pairs: int, nmin: int, nmax: int, seed: int = 1):
    import twoview_cases as cases

    rng = np.random.default_rng(seed)
    parts = [cases.scene(rng, int(rng.integers(nmin, nmax + 1)), outliers=rng.uniform(0.0, 0.6)) for _ in range(pairs)]
    b1 = np.concatenate([p[0] for p in parts])
    b2 = np.concatenate([p[1] for p in parts])
    off = np.r_[0, np.cumsum([len(p[0]) for p in parts])].astype(np.int64)
    return b1, b2, off


def stats(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--nmin", type=int, default=50)
    ap.add_argument("--nmax", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--cpu-pairs", type=int, default=48)
    a = ap.parse_args()
    ctx = default_context()
    b1, b2, off = workload(a.pairs, a.nmin, a.nmax)
    res, _, _ = matching.relpose_pairs(b1, b2, off, THRESHOLD, mode="ransac", ctx=ctx)  # warm-up of the rounds, and the poses of `finish`
    poses = np.array([np.r_[r["lo_model"][:, :3].T.reshape(9), -r["lo_model"][:, :3].T.dot(r["lo_model"][:, 3])] for r in res])
    calls = {
        "ransac_alone": lambda: matching.relpose_pairs(b1, b2, off, THRESHOLD, mode="ransac", ctx=ctx),
        "two_view": lambda: reconstruction.two_view_pairs(b1, b2, off, THRESHOLD, check_reversal=False, ctx=ctx),
        "two_view_reversal": lambda: reconstruction.two_view_pairs(b1, b2, off, THRESHOLD, check_reversal=True, reversal_ratio=0.95, ctx=ctx),
        "finish": lambda: reconstruction.two_view_pairs(b1, b2, off, THRESHOLD, poses=poses, check_reversal=False, ctx=ctx),
        "finish_reversal": lambda: reconstruction.two_view_pairs(b1, b2, off, THRESHOLD, poses=poses, check_reversal=True, reversal_ratio=0.95, ctx=ctx),
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
    out = {"workload": f"{a.pairs} pairs, N in [{a.nmin}, {a.nmax}] ({int(off[-1])} correspondences), mismatches 0-0.6", "steps": a.steps}
    for name in calls:
        out[name] = {"kernel_ms": stats(kernel_ms[name]), "wall_ms": stats(wall_ms[name])}
    for name in ("two_view", "two_view_reversal"):
        r = last[name][0]
        its = np.array([x["refine_iterations"][: 2 if name.endswith("reversal") else 1] for x in r], np.float64)
        status = np.array([x["status"] for x in r])
        out[name]["mean_refine_iterations"] = [float(v) for v in its.mean(axis=0)]
        out[name]["status_counts"] = {s: int((status == k).sum()) for k, s in enumerate(reconstruction.TWO_VIEW_STATUS)}
        out[name]["pairs_per_s_end_to_end"] = a.pairs / (out[name]["wall_ms"]["median"] / 1e3)
    # the host build of the same header on one thread, a sample of the same pairs, RANSAC included
    import twoview_cases as cases

    lib = cases.build_host()
    m = min(a.cpu_pairs, a.pairs)
    for name, reversal in (("host_one_thread", False), ("host_one_thread_reversal", True)):
        t0 = time.perf_counter()
        cases.host_pairs(lib, b1[: off[m]], b2[: off[m]], off[: m + 1], None, THRESHOLD, reversal, 0.95)
        cpu = time.perf_counter() - t0
        t0 = time.perf_counter()
        cases.host_pairs(lib, b1[: off[m]], b2[: off[m]], off[: m + 1], poses[:m], THRESHOLD, reversal, 0.95)
        cpu_finish = time.perf_counter() - t0
        out[name] = {"pairs": m, "ms_per_pair": 1e3 * cpu / m, "finish_ms_per_pair": 1e3 * cpu_finish / m,
                     "batch_of_%d_would_take_ms" % a.pairs: 1e3 * cpu / m * a.pairs}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
