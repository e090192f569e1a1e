"""opensfm_amd.compat.pydense: the class and method names of the reference's dense/python/pybind.cc, the opt-in registration, and the
default ``install()`` left as it was (no GPU needed; the calls are exercised in tests/test_gpu_depthmap.py)."""
import inspect
import json
import os
import re
import sys
import types

import pytest

from opensfm_amd import compat

REF = "/root/reference/opensfm/src"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pydense_names.json")


def pydense_names(ref: str) -> dict:
    """class -> method names of dense/python/pybind.cc (stored in tests/golden/pydense_names.json: run this file to write it)"""
    text = open(os.path.join(ref, "dense/python/pybind.cc")).read()
    names = {}
    for block in text.split("py::class_<")[1:]:
        cls = re.search(r'\(m,\s*"(\w+)"\)', block).group(1)
        names[cls] = sorted(set(re.findall(r'\.def\(\s*"(\w+)"', block)))
    return names


def test_names_are_those_of_the_reference():
    names = json.load(open(GOLDEN))
    if os.path.isdir(REF):
        assert pydense_names(REF) == names, "tests/golden/pydense_names.json is stale: run tests/test_compat_pydense.py as a script"
    for cls in ("DepthmapEstimator", "DepthmapCleaner"):
        ours = {n for n, f in inspect.getmembers(getattr(compat.pydense, cls), callable) if not n.startswith("_")}
        assert ours == set(names[cls]), (cls, sorted(ours ^ set(names[cls])))
    assert isinstance(compat.pydense.DepthmapEstimator.seed, property)  # the one addition
    # the argument order of depthmap_bind.h
    assert list(inspect.signature(compat.pydense.DepthmapEstimator.add_view).parameters) == ["self", "K", "R", "t", "image", "mask"]
    assert list(inspect.signature(compat.pydense.DepthmapEstimator.set_depth_range).parameters) == ["self", "min_depth", "max_depth", "num_depth_planes"]
    assert list(inspect.signature(compat.pydense.DepthmapCleaner.add_view).parameters) == ["self", "K", "R", "t", "depth"]
    # not provided
    assert {"DepthmapPruner", "OpenMVSExporter"} <= set(names)
    for missing in ("DepthmapPruner", "OpenMVSExporter"):
        assert not hasattr(compat.pydense, missing)


def test_seed_defaults_to_a_fixed_value_and_shapes_must_match():
    import numpy as np

    from opensfm_amd import dense

    a, b = compat.pydense.DepthmapEstimator(), compat.pydense.DepthmapEstimator()
    assert a.seed == b.seed == dense.DEFAULT_SEED
    a.seed = 5
    assert a.seed == 5 and b.seed == dense.DEFAULT_SEED
    with pytest.raises(ValueError, match="image and mask must have matching shapes"):
        a.add_view(np.eye(3), np.eye(3), np.zeros(3), np.zeros((4, 5), np.uint8), np.zeros((4, 6), np.uint8))


def test_registration_is_opt_in():
    pkg = types.ModuleType("osfm_dense_probe")
    sys.modules["osfm_dense_probe"] = pkg
    try:
        done = compat.install("osfm_dense_probe")
        assert sorted(done) == ["pybundle", "pyfeatures", "pyrobust", "pysfm"] and "osfm_dense_probe.pydense" not in sys.modules
        done = compat.install("osfm_dense_probe", extra=("pydense",))
        assert sorted(done) == ["pydense"]
        from osfm_dense_probe import pydense

        assert pydense.DepthmapEstimator is compat.pydense.DepthmapEstimator and pkg.pydense is pydense
        for missing in ("DepthmapPruner", "OpenMVSExporter"):
            with pytest.raises(AttributeError, match=missing):
                getattr(pydense, missing)
        with pytest.raises(ValueError, match="pymap"):
            compat.install("osfm_dense_probe", extra=("pymap",))
    finally:
        for k in [k for k in sys.modules if k.startswith("osfm_dense_probe")]:
            del sys.modules[k]
    pkg = types.ModuleType("osfm_dense_probe2")
    sys.modules["osfm_dense_probe2"] = pkg
    try:
        assert sorted(compat.install_dense("osfm_dense_probe2")) == ["pybundle", "pydense", "pyfeatures", "pyrobust", "pysfm"]
    finally:
        for k in [k for k in sys.modules if k.startswith("osfm_dense_probe2")]:
            del sys.modules[k]


if __name__ == "__main__":
    json.dump(pydense_names(REF), open(GOLDEN, "w"), indent=1)
