"""Measurement of depthmap pruning and merging (osfm_depthmap_prune, prune.hip) on one MI355X.  Not part of bench.py's headline line.

Workload (defaults): a batch of 64 shots of 640 x 480 with 1 + 9 views each -- the rendered depths of tests/depthmap_cases.clean_problem
(zeros included; the other views are 643 x 478) with the planes, colours and labels of tests/prune_cases.py, made once and used for
every shot of the batch --, same_depth_threshold 0.01.

    python tools/prune_bench.py [--shots 64] [--width 640] [--height 480] [--views 10] [--steps 3] [--warmup 1] [--hbm-tbs 8.0] [--no-host]

Prints one JSON line.  After --warmup untimed calls of the same batch, the median over --steps calls, with the smallest and largest in
brackets: kernel milliseconds per shot (HIP events; the sum of the three kernels, and mark / scan / scatter apart), end-to-end
milliseconds per shot of ``dense.prune_raw`` (packing, uploads and the download of the kept rows included), the rows kept, and what
fraction of the HBM bound the kernel time amounts to.  The bound counts the bytes the three kernels must move: every depth and plane of
every view once (16 B per pixel), the colour and label of the first view once (4 B per pixel), the keep flag written and read again
(2 B per first-view pixel), the block counts and offsets (20 B per 256 first-view pixels), and per kept row the depth and plane read
again by the scatter (16 B) and the four outputs (28 B) -- at --hbm-tbs.  "host": ONE shot of the batch through the HOST BUILD of
prune.hip (tests/native/build_prune_emu.py: the same kernels on one CPU thread, lanes as fibres) -- a port made for testing, NOT the
reference and not an optimised CPU implementation -- in milliseconds per shot, with whether its rows equal the GPU's."""
from __future__ import annotations

import argparse
import ctypes as C
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prune_cases as cases  # noqa: E402
from opensfm_amd import _lib, dense  # noqa: E402


def median_min_max(values):
    return [float(np.median(values)), float(min(values)), float(max(values))]


def run(problems, params, steps, warmup):
    split, total, out = [], [], None
    for _ in range(warmup):  # the timed shape itself: the kernels' first launch and the pool block stay outside the window
        dense.prune_raw(problems, params)
    ms3 = (C.c_double * 3)()
    for _ in range(steps):
        t0 = time.perf_counter()
        out = dense.prune_raw(problems, params)
        total.append((time.perf_counter() - t0) * 1e3)
        _lib.check(_lib.load().osfm_depthmap_prune_split_ms(_lib.default_context().handle, ms3), "osfm_depthmap_prune_split_ms")
        split.append(list(ms3))
    return np.asarray(split), total, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=64)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    problem = cases.prune_problem(args.views, args.width, args.height, behind=False)
    problems = [problem] * args.shots
    params = dense.params_from_config({"depthmap_same_depth_threshold": 0.01})
    dense.prune_raw([cases.prune_problem(2, 16, 16, False)], params)  # context, pool
    split, total, (merged, counts, _) = run(problems, params, args.steps, args.warmup)
    rows = int(counts.sum())
    first = args.width * args.height
    bytes_per_shot = 16 * sum(v[3].size for v in problem["views"]) + 4 * first + 2 * first + 20 * ((first + 255) // 256) + 44 * int(counts[0])
    kernel = split.sum(axis=1)
    per_shot = lambda values: [v / args.shots for v in median_min_max(values)]  # noqa: E731
    result = {"shots": args.shots, "size": [args.width, args.height], "views": args.views, "steps": args.steps, "warmup": args.warmup,
              "rows_kept": rows, "rows_kept_per_shot": int(counts[0]), "live_pixels_per_shot": cases.live_pixels(problem["views"]),
              "kernel_ms_per_shot_median_min_max": per_shot(kernel),
              "mark_ms_per_shot_median_min_max": per_shot(split[:, 0]), "scan_ms_per_shot_median_min_max": per_shot(split[:, 1]),
              "scatter_ms_per_shot_median_min_max": per_shot(split[:, 2]),
              "end_to_end_ms_per_shot_median_min_max": per_shot(total),
              "shots_per_s_kernel": args.shots / (float(np.median(kernel)) * 1e-3), "shots_per_s_end_to_end": args.shots / (float(np.median(total)) * 1e-3),
              "hbm_bytes_per_shot": bytes_per_shot,
              "fraction_of_hbm_bound": bytes_per_shot * args.shots / (args.hbm_tbs * 1e12) / (float(np.median(kernel)) * 1e-3)}
    if not args.no_host:
        gpu_one = dense.prune_raw([problem], params)
        spec = importlib.util.spec_from_file_location("build_prune_emu", os.path.join(ROOT, "tests", "native", "build_prune_emu.py"))
        builder = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(builder)
        lib = C.CDLL(builder.build())
        for name, (res, argtypes) in _lib._signatures().items():
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, argtypes
        # the GPU library and its contexts stay alive and come back afterwards: a context must be destroyed by the library that made it
        gpu_lib, gpu_ctx = _lib._lib, getattr(_lib._tls, "ctx", None)
        _lib._lib, _lib._tls.ctx = lib, {}
        try:
            t0 = time.perf_counter()
            host_one = dense.prune_raw([problem], params)
            seconds = time.perf_counter() - t0
            result["host"] = {"what": "the host build of the same kernels on one thread: a port made for testing, not the reference",
                              "end_to_end_ms_per_shot": seconds * 1e3, "equal_to_gpu": bool(cases.same_cloud(host_one[0], gpu_one[0]))}
        finally:
            for ctx in _lib._tls.ctx.values():
                ctx.close()
            _lib._lib, _lib._tls.ctx = gpu_lib, gpu_ctx
    print(json.dumps(result))


if __name__ == "__main__":
    main()
