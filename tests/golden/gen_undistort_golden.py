"""Writes tests/golden/undistort/*.npz: the results of the plain restatement of image undistortion (tests/undistort_cases.py) -- every remap
case in the four modes, the camera mappings of every case at both sizes, and the six views of the panorama.  No GPU and no library is
needed; the inputs are regenerated from the seeds of the case module.  tests/test_undistort_host.py regenerates and compares;
tests/test_gpu_undistort.py reads them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import undistort_cases as cases  # noqa: E402


def remap_results(name):
    src, map1, map2 = cases.remap_case(name)
    return {mode: cases.remap(src, map1, map2, interpolation, border) for mode, (interpolation, border) in cases.MODES.items()}


def mapping_results(width, height):
    out = {}
    for name in cases.mapping_names(width, height):
        from_cam, to_cam = cases.MAPPING_CASES[name]
        out[name + "_map1"], out[name + "_map2"] = cases.camera_mapping(from_cam, to_cam, width, height)
    return out


def panorama_results():
    P = cases.PANORAMA
    image, R_pano = cases.panorama_image(), cases.panorama_pose_rotation()
    view_cam = ("perspective", [0.0, 0.0, 0.5])
    out = {}
    for name, R_view in zip(cases.VIEW_NAMES, cases.view_rotations()):
        x, y = cases.panorama_view_mapping(np.dot(R_pano, R_view.T), view_cam, P["view"], P["view"], P["pano_w"], P["pano_h"])
        out[name + "_x"], out[name + "_y"] = x, y
        out[name + "_linear"] = cases.remap(image, x, y, cases.INTER_LINEAR, cases.BORDER_WRAP)
        out[name + "_nearest"] = cases.remap(image, x, y, cases.INTER_NEAREST, cases.BORDER_WRAP)
    return out


def generate():
    os.makedirs(cases.GOLDEN, exist_ok=True)
    for name in cases.REMAP_CASES:
        np.savez_compressed(os.path.join(cases.GOLDEN, "remap_" + name + ".npz"), **remap_results(name))
        print("remap", name, flush=True)
    for width, height in cases.MAPPING_SIZES:
        np.savez_compressed(os.path.join(cases.GOLDEN, f"mapping_{width}x{height}.npz"), **mapping_results(width, height))
        print("mapping", width, height, flush=True)
    np.savez_compressed(os.path.join(cases.GOLDEN, "panorama.npz"), **panorama_results())
    print("panorama", flush=True)


if __name__ == "__main__":
    generate()
