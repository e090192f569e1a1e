"""Driven by tests/test_native_sanitizers.py: two LM iterations of the emulated bundle-adjustment solver (the real ba.hip / ba_generic.inc on
tests/native/hipemu) over four small scenes, cost histories saved to an .npz.  argv: plain | asan, the output file.  With `asan` the library is the
-fsanitize=address,undefined build and the caller has put the sanitizer runtime into LD_PRELOAD: an out-of-bounds index into a __shared__ array, a
kernel's local array or a device buffer ends the process with a report instead of corrupting a neighbour silently, as it would on the GPU."""
import os
import sys

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
import numpy as np

from emu_util import emulated
from opensfm_amd import bundle, synthetic

NO_TOL = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
ITERS = {"bundle_max_iterations": 2}


def scenes():
    """name, solver, problem"""
    yield "k1_k2_focal", bundle.bundle_arrays, synthetic.make_ba_scene(20, 300, 5)
    local = bundle.local_problem(synthetic.make_ba_scene(40, 500, 6, seed=7), 20,
                                 {"local_bundle_radius": 3, "local_bundle_min_common_points": 20, "local_bundle_max_shots": 8})[0]
    assert local["cam_fixed"].all()
    yield "local_constant_cameras", bundle.bundle_arrays, local
    yield "generic_brown", bundle.bundle_general_arrays, synthetic.make_bundle_scene(models=("brown",), n_instances=8, n_points=100, rig=False, gps=False,
                                                                                    n_gcp=0, up_vectors=False, seed=7)
    yield "rig_bias_control_points_up_vectors", bundle.bundle_general_arrays, synthetic.make_bundle_scene(models=("perspective", "brown"), n_instances=8,
                                                                                                         n_points=90, seed=5)


def main(mode: str, out: str) -> None:
    res = {}
    with emulated(sanitize=mode == "asan") as lib:
        for name, solve, pr in scenes():
            g = solve(pr, ITERS, **NO_TOL)
            assert g["iterations"] == 2, (name, g["iterations"])
            res[name] = np.asarray(g["cost_history"])
            print("%s: %d launches so far, cost %r" % (name, lib.hipemu_launch_count(), res[name].tolist()), flush=True)
    np.savez(out, **res)
    print("emulated bundle adjustment (%s): clean" % mode)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
