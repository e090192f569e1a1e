"""Measurement of the rotation-only LO-RANSAC of compute_image_pairs (osfm_relrot_pairs, relrot.hip) on one MI355X, next to the host
build of the same header (tests/native/relrot_host.cpp) on 16 threads.  Not part of bench.py's headline line.

Workload (defaults): 20 000 pairs, N uniform in [50, 2000] correspondences, outlier fractions uniform in [0, 0.8], half of the pairs
pure rotations and half with a baseline; threshold 0.016 (4 x five_point_algo_threshold), 1000 iterations, probability 0.99, LO on,
the rotation-only inlier count on (what compute_image_pairs asks for).

    python tools/relrot_bench.py [--pairs 20000] [--nmin 50] [--nmax 2000] [--steps 3] [--cpu-pairs 2000]

Reports pairs / s and kernel ms (HIP events), hypotheses evaluated (main + LO models scored) and point evaluations / s, and the host
build's pairs / s on a sample of the same pairs with 16 threads.  Meant also for `rocprofv3 --kernel-trace --stats -- python ...`."""
from __future__ import annotations

import argparse
import concurrent.futures as cf
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


def workload(pairs: int, nmin: int, nmax: int, seed: int = 1):
    from test_relrot_host import make_problem

    rng = np.random.default_rng(seed)
    parts = [make_problem(rng, int(rng.integers(nmin, nmax + 1)), outliers=rng.uniform(0.0, 0.8), baseline=(0.0 if k % 2 == 0 else rng.uniform(0.2, 1.5)))
             for k in range(pairs)]
    b1 = np.concatenate([p[0] for p in parts])
    b2 = np.concatenate([p[1] for p in parts])
    off = np.r_[0, np.cumsum([len(p[0]) for p in parts])].astype(np.int64)
    return b1, b2, off


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20000)
    ap.add_argument("--nmin", type=int, default=50)
    ap.add_argument("--nmax", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--cpu-pairs", type=int, default=2000)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    ctx = default_context()
    b1, b2, off = workload(a.pairs, a.nmin, a.nmax)
    reconstruction.relrot_pairs(b1[: off[8]], b2[: off[8]], off[:9], 0.016, inlier_chord=0.016, ctx=ctx)  # warm-up
    kms, walls = [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        res, _, ms = reconstruction.relrot_pairs(b1, b2, off, 0.016, inlier_chord=0.016, ctx=ctx)
        walls.append(time.perf_counter() - t0)
        kms.append(ms)
    n = np.diff(off)
    iters = np.array([r["iterations"] for r in res], np.float64)
    # models scored: one per iteration; the LO models are not counted per pair by the kernel, so the count is a lower bound
    hyp = float(iters.sum())
    point_evals = float((iters * n).sum())
    k_ms = float(np.median(kms))
    out = {"workload": f"{a.pairs} pairs, N in [{a.nmin}, {a.nmax}], outliers 0-0.8, half pure rotations",
           "kernel_ms": k_ms, "wall_ms": 1e3 * float(np.median(walls)), "pairs_per_s": a.pairs / (k_ms / 1e3),
           "hypotheses_main": hyp, "point_evals_main_per_s": point_evals / (k_ms / 1e3),
           "mean_iterations": float(iters.mean()), "pairs_positive_score": int(sum(r["reconstructability"] > 0 for r in res))}
    # the host build of the same header, a sample of the same pairs split over `threads` threads (the walk releases the GIL in ctypes)
    from test_relrot_host import build_host, host_pairs

    lib = build_host()
    m = min(a.cpu_pairs, a.pairs)
    chunks = np.array_split(np.arange(m), a.threads)

    def run(ch):
        if len(ch) == 0:
            return 0
        lo, hi = int(off[ch[0]]), int(off[ch[-1] + 1])
        host_pairs(lib, b1[lo:hi], b2[lo:hi], off[ch[0]: ch[-1] + 2] - lo, 0.016, chord=0.016)
        return len(ch)

    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(a.threads) as ex:
        done = sum(ex.map(run, chunks))
    cpu = time.perf_counter() - t0
    out.update({"cpu_threads": a.threads, "cpu_pairs": done, "cpu_pairs_per_s": done / cpu})
    out["speedup_vs_cpu"] = out["pairs_per_s"] / out["cpu_pairs_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
