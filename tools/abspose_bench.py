"""Measurement of the absolute-pose LO-RANSAC of resect (osfm_abspose_images, abspose.hip) on one MI355X, next to the host build of the
same header (tests/native/abspose_host.cpp) on 16 threads.  Not part of bench.py's headline line.

Two workloads: one call of the size resect_candidates makes (8 images of 50 - 2 000 rows), and one large batch (default 2 000 images of
50 - 2 000 rows); outlier fractions uniform in [0, 0.6], bearing noise 1e-3, threshold 0.004 (resection_threshold), 1000 iterations,
probability 0.99, LO on, resect's inlier test on.

    python tools/abspose_bench.py [--images 2000] [--nmin 50] [--nmax 2000] [--steps 3] [--cpu-images 256]

Reports for each: kernel ms (HIP events), end-to-end ms of the call, images / s, and the host build's images / s on (a sample of) the
same images with 16 threads.  The path is new, so there is no earlier GPU time to compare with: the comparison is the host build."""
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
from opensfm_amd import reconstruction  # noqa: E402
from opensfm_amd._lib import default_context  # noqa: E402

THRESHOLD = 0.004


def workload(images: int, nmin: int, nmax: int, seed: int = 1):
    import abspose_cases as cases

    rng = np.random.default_rng(seed)
    return cases.pack([cases.make_problem(rng, int(rng.integers(nmin, nmax + 1)), "noisy", outliers=rng.uniform(0.0, 0.6)) for _ in range(images)])


def measure(name: str, b, X, off, steps: int, cpu_images: int, threads: int, ctx) -> dict:
    from test_abspose_host import build_host, host_images_threads

    images = len(off) - 1
    kms, walls = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        res, _, _, ms = reconstruction.abspose_images(b, X, off, THRESHOLD, ctx=ctx)
        walls.append(time.perf_counter() - t0)
        kms.append(ms)
    k_ms, wall_ms = float(np.median(kms)), 1e3 * float(np.median(walls))
    iters = np.array([r["iterations"] for r in res], np.float64)
    out = {"workload": name, "images": images, "rows": int(off[-1]), "kernel_ms": k_ms, "wall_ms": wall_ms,
           "images_per_s_kernel": images / (k_ms / 1e3), "images_per_s_wall": images / (wall_ms / 1e3), "mean_iterations": float(iters.mean())}
    m = min(cpu_images, images)
    lib = build_host()
    t0 = time.perf_counter()
    host_images_threads(lib, b[: off[m]], X[: off[m]], off[: m + 1], THRESHOLD, threads=min(threads, m))
    cpu = time.perf_counter() - t0
    out.update({"cpu_threads": min(threads, m), "cpu_images": m, "cpu_ms": 1e3 * cpu, "cpu_images_per_s": m / cpu})
    out["speedup_vs_cpu_wall"] = out["images_per_s_wall"] / out["cpu_images_per_s"]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--nmin", type=int, default=50)
    ap.add_argument("--nmax", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--cpu-images", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    ctx = default_context()
    b, X, off = workload(a.images, a.nmin, a.nmax)
    reconstruction.abspose_images(b[: off[2]], X[: off[2]], off[:3], THRESHOLD, ctx=ctx)  # warm-up
    small = measure(f"one resect_candidates call: 8 images, N in [{a.nmin}, {a.nmax}]", b[: off[8]], X[: off[8]], off[:9], a.steps, 8, a.threads, ctx)
    print(json.dumps(small))
    large = measure(f"{a.images} images, N in [{a.nmin}, {a.nmax}], outliers 0-0.6", b, X, off, a.steps, a.cpu_images, a.threads, ctx)
    print(json.dumps(large))


if __name__ == "__main__":
    main()
