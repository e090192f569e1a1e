"""Measurement of the depthmap estimator and cleaner (osfm_depthmap_estimate / osfm_depthmap_clean, depthmap.hip) on one MI355X.  Not part
of bench.py's headline line.

Workload (defaults): a batch of 64 shots of 640 x 480 with 1 + 9 views each (the synthetic scene of tests/depthmap_cases.py, rendered once
and used for every shot of the batch), patch 7, three PatchMatch iterations or 100 planes, each method in turn.

    python tools/depthmap_bench.py [--shots 64] [--width 640] [--height 480] [--views 10] [--methods BRUTE_FORCE,PATCH_MATCH,PATCH_MATCH_SAMPLE]
                                   [--steps 3] [--warmup 1] [--no-host]

Prints one JSON line.  Per method, after --warmup untimed calls of the same batch, the median over --steps calls (and the smallest and
largest kernel time): kernel milliseconds per shot (HIP events), end-to-end milliseconds per shot of the array call
(uploads and downloads included), shots per second of both, the NOMINAL bilinear samples per second -- interior pixels x candidates x
views x patch area, every candidate counted as evaluated: an upper bound on the work, ignored pixels and skipped candidates included --
and what fraction of two bounds the kernel time amounts to: fp32 VALU (--flops-per-sample, 40 by default: two coordinates, four taps,
three lerps, the weight look-up and eleven NCC operations; 157.3 TFLOP/s) and HBM (every image, mask and output once, at --hbm-tbs).
"host": a 48 x 40, 3-view problem through the HOST BUILD of depthmap.hip (tests/native/build_depthmap_emu.py: the same kernels on one
CPU thread, lanes as fibres) -- a port made for testing, NOT the reference and not an optimised CPU implementation -- in nominal samples
per second, with whether its results equal the GPU's."""
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
import depthmap_cases as cases  # noqa: E402
from opensfm_amd import _lib, dense  # noqa: E402


def nominal_samples(method: str, w: int, h: int, views: int, patch: int, iterations: int, planes: int) -> float:
    interior = max(w - patch + 1, 0) * max(h - patch + 1, 0)
    others = views - 1
    if method == "BRUTE_FORCE":
        scores = planes * others
    elif method == "PATCH_MATCH":
        scores = others + 2 * iterations * 8 * others
    else:
        scores = 1 + 2 * iterations * (8 + (1 if views > 2 else 0))
    return float(interior) * scores * patch * patch


def run(problems, method, args, seed=1):
    p = dense.params_from_config({"depthmap_method": method, "depthmap_patch_size": args.patch, "depthmap_patchmatch_iterations": args.iterations},
                                 num_depth_planes=args.planes)
    kernel, total, out = [], [], None
    for _ in range(getattr(args, "warmup", 0)):  # the timed shape itself: the kernel's first launch and the pool block stay outside the window
        dense.estimate_raw(problems, p, seed)
    for _ in range(args.steps):
        t0 = time.perf_counter()
        out, ms = dense.estimate_raw(problems, p, seed)
        total.append((time.perf_counter() - t0) * 1e3)
        kernel.append(ms)
    return float(np.median(kernel)), float(np.median(total)), out, [float(min(kernel)), float(max(kernel))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=64)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--patch", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--planes", type=int, default=100)
    ap.add_argument("--methods", default="BRUTE_FORCE,PATCH_MATCH,PATCH_MATCH_SAMPLE")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--flops-per-sample", type=float, default=40.0)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    problem = cases.make_problem(args.width, args.height, args.views)
    problems = [problem] * args.shots
    result = {"shots": args.shots, "size": [args.width, args.height], "views": args.views, "patch": args.patch, "iterations": args.iterations,
              "planes": args.planes}
    bytes_per_shot = sum(v[3].size for v in problem["views"]) + problem["views"][0][4].size + 24 * args.width * args.height
    dense.estimate_raw([cases.make_problem(16, 16, 2)], dense.params_from_config(None, method=0, patch_size=3), 1)  # context, pool, tables
    for method in args.methods.split(","):
        kernel, total, _, spread = run(problems, method, args)
        samples = nominal_samples(method, args.width, args.height, args.views, args.patch, args.iterations, args.planes) * args.shots
        result[method] = {"kernel_ms_per_shot": kernel / args.shots, "kernel_ms_per_shot_min_max": [v / args.shots for v in spread], "end_to_end_ms_per_shot": total / args.shots,
                          "shots_per_s_kernel": args.shots / (kernel * 1e-3), "shots_per_s_end_to_end": args.shots / (total * 1e-3),
                          "nominal_samples_per_s": samples / (kernel * 1e-3),
                          "fraction_of_fp32_valu_bound": samples * args.flops_per_sample / 157.3e12 / (kernel * 1e-3),
                          "fraction_of_hbm_bound": bytes_per_shot * args.shots / (args.hbm_tbs * 1e12) / (kernel * 1e-3)}
    if not args.no_host:
        small = cases.make_problem(48, 40, 3)
        small_args = argparse.Namespace(patch=args.patch, iterations=1, planes=8, steps=1)
        gpu = {m: run([small], m, small_args)[2] for m in args.methods.split(",")}
        spec_path = os.path.join(ROOT, "tests", "native", "build_depthmap_emu.py")
        import importlib.util

        spec = importlib.util.spec_from_file_location("build_depthmap_emu", spec_path)
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
        result["host"] = {"what": "the host build of the same kernels on one thread: a port made for testing, not the reference"}
        try:
            for method in args.methods.split(","):
                t0 = time.perf_counter()
                out = run([small], method, small_args)[2]
                seconds = time.perf_counter() - t0
                equal = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(out[0], gpu[method][0]))
                result["host"][method] = {"nominal_samples_per_s": nominal_samples(method, 48, 40, 3, args.patch, 1, 8) / seconds,
                                          "equal_to_gpu": bool(equal)}
        finally:
            for ctx in _lib._tls.ctx.values():
                ctx.close()
            _lib._lib, _lib._tls.ctx = gpu_lib, gpu_ctx
    print(json.dumps(result))


if __name__ == "__main__":
    main()
