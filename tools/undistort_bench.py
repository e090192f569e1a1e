"""Measurement of image undistortion (osfm_undistort_images, osfm_camera_mapping + osfm_remap_images, undistort.hip) on one MI355X.  Not
part of bench.py's headline line.

Workload (defaults): a batch of 64 Brown-camera images of 2048 x 1536 x 3 that share two cameras -- "linear": the images with linear
interpolation at full size; "linear_max_size": the same images with scale_image(max_size 1024) folded in; "nearest_masks": one-channel
masks with nearest interpolation -- each through the fused call and through map-then-remap (two maps, uploaded once each).

    python tools/undistort_bench.py [--images 64] [--width 2048] [--height 1536] [--max-size 1024] [--steps 3] [--warmup 1] [--no-host]

Prints one JSON line.  Per variant and path, after --warmup untimed calls of the same batch, the median over --steps calls (and the
smallest and largest): kernel milliseconds per image (HIP events around the kernel), end-to-end milliseconds per image of the array call
(uploads and downloads included), and the kernel time's share of the HBM bound: the bytes the kernel must move -- every output pixel
written once, every source pixel read once (the pixels of a scaled output read four taps each: counted as min(source, 4 x output)), for
map-then-remap the two maps read at the output pixels -- over --hbm-tbs (8.0 TB/s, the HBM3E peak of MI355X_MICROARCH.md).  The
map-then-remap figures are those of the remap call alone; "mapping" reports the two maps' kernel time separately.
"host": a 256 x 192 x 3 image through the HOST BUILD of undistort.hip (tests/native/build_undistort_emu.py: the same kernels on one CPU
thread) -- a port made for testing, NOT cv2 (which cannot run here) and not an optimised CPU implementation -- in milliseconds per
megapixel, with whether its bytes equal the GPU's."""
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
from opensfm_amd import _lib, undistort  # noqa: E402
from opensfm_amd.geometry_types import Camera  # noqa: E402


def brown_cameras(width, height):
    cams = []
    for k, (k1, focal) in enumerate(((-0.12, 0.85), (-0.08, 0.78))):
        c = Camera.create_brown(focal, 1.002, [0.003, -0.002], [k1, 0.02, -0.001, 0.0004, -0.0003])
        c.id, c.width, c.height = f"cam{k}", width, height
        cams.append(c)
    return cams, [undistort.undistorted_camera(c) for c in cams]


def timed(call, steps, warmup):
    for _ in range(warmup):  # the timed shape itself: first launches and the pool block stay outside the window
        call()
    kernel, total, out = [], [], None
    for _ in range(steps):
        t0 = time.perf_counter()
        out, ms = call()
        total.append((time.perf_counter() - t0) * 1e3)
        kernel.append(ms)
    return out, {"kernel_ms": float(np.median(kernel)), "kernel_ms_min_max": [float(min(kernel)), float(max(kernel))],
                 "end_to_end_ms": float(np.median(total))}


def per_image(t, n, bytes_moved, hbm_tbs):
    return {"kernel_ms_per_image": t["kernel_ms"] / n, "kernel_ms_per_image_min_max": [v / n for v in t["kernel_ms_min_max"]],
            "end_to_end_ms_per_image": t["end_to_end_ms"] / n, "kernel_bytes": int(bytes_moved),
            "fraction_of_hbm_bound": bytes_moved / (hbm_tbs * 1e12) / (t["kernel_ms"] * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--height", type=int, default=1536)
    ap.add_argument("--max-size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    n, w, h = args.images, args.width, args.height
    rng = np.random.default_rng(1)
    froms, tos = brown_cameras(w, h)
    cam_of = [k % 2 for k in range(n)]
    distinct = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(min(n, 4))]  # (host memory: four distinct images, repeated)
    images = [distinct[k % len(distinct)] for k in range(n)]
    masks = [np.ascontiguousarray(im[:, :, 0] > 127).astype(np.uint8) * 255 for im in distinct]
    masks = [masks[k % len(masks)] for k in range(n)]
    scaled = undistort.scale_image_size(h, w, args.max_size)
    result = {"images": n, "size": [w, h], "max_size": args.max_size, "scaled_size": [scaled[1], scaled[0]], "hbm_tbs": args.hbm_tbs}
    undistort.undistort_raw([distinct[0][:16, :16]], [0], froms, tos, undistort.INTER_AREA)  # context, pool
    maps, t = timed(lambda: undistort.compute_camera_mappings([(froms[k], tos[k], w, h) for k in range(2)]), args.steps, args.warmup)
    result["mapping"] = {"kernel_ms_per_map": t["kernel_ms"] / 2, "kernel_ms_per_map_min_max": [v / 2 for v in t["kernel_ms_min_max"]],
                         "end_to_end_ms_per_map": t["end_to_end_ms"] / 2}
    image_maps = [maps[c] for c in cam_of]
    variants = (("linear", images, undistort.INTER_AREA, None, 3), ("linear_max_size", images, undistort.INTER_AREA, scaled, 3),
                ("nearest_masks", masks, undistort.INTER_NEAREST, None, 1))
    for name, batch, interpolation, size, channels in variants:
        sizes = None if size is None else [size] * n
        out_px = (size[0] * size[1]) if size else w * h
        pixel_bytes = n * channels * (out_px + min(w * h, 4 * out_px))
        fused, tf = timed(lambda: undistort.undistort_raw(batch, cam_of, froms, tos, interpolation, sizes), args.steps, args.warmup)
        two, tr = timed(lambda: undistort.remap_raw(batch, image_maps, interpolation, undistort.BORDER_CONSTANT, sizes), args.steps, args.warmup)
        result[name] = {"fused": per_image(tf, n, pixel_bytes, args.hbm_tbs), "map_then_remap": per_image(tr, n, pixel_bytes + n * out_px * 8, args.hbm_tbs),
                        "fused_equals_map_then_remap": bool(all(np.array_equal(a, b) for a, b in zip(fused, two)))}
    if not args.no_host:
        hw, hh = 256, 192
        hf, ht = brown_cameras(hw, hh)
        small = np.ascontiguousarray(distinct[0][:hh, :hw])
        gpu, _ = undistort.undistort_raw([small], [0], hf, ht, undistort.INTER_AREA)
        spec = importlib.util.spec_from_file_location("build_undistort_emu", os.path.join(ROOT, "tests", "native", "build_undistort_emu.py"))
        builder = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(builder)
        lib = C.CDLL(builder.build())
        for fname, (res, argtypes) in _lib._signatures().items():
            if hasattr(lib, fname):
                fn = getattr(lib, fname)
                fn.restype, fn.argtypes = res, argtypes
        # the GPU library and its contexts stay alive and come back afterwards: a context must be destroyed by the library that made it
        gpu_lib, gpu_ctx = _lib._lib, getattr(_lib._tls, "ctx", None)
        _lib._lib, _lib._tls.ctx = lib, {}
        try:
            t0 = time.perf_counter()
            host, _ = undistort.undistort_raw([small], [0], hf, ht, undistort.INTER_AREA)
            seconds = time.perf_counter() - t0
            result["host"] = {"what": "the host build of the same kernels on one thread: a port made for testing, not cv2",
                              "size": [hw, hh], "ms_per_megapixel": seconds * 1e3 / (hw * hh / 1e6), "equal_to_gpu": bool(np.array_equal(host[0], gpu[0]))}
        finally:
            for ctx in _lib._tls.ctx.values():
                ctx.close()
            _lib._lib, _lib._tls.ctx = gpu_lib, gpu_ctx
    print(json.dumps(result))


if __name__ == "__main__":
    main()
