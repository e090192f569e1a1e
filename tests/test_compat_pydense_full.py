"""opensfm_amd.compat.pydense_full: ``pydense`` with ``DepthmapPruner`` -- the method names of the reference's dense/python/pybind.cc, the
wrapper's argument order and messages, its registration AS ``<package>.pydense``, and what ``install()`` / ``install_dense()`` register
left as it was (no GPU needed; the calls are exercised in tests/test_prune_host.py and tests/test_gpu_prune.py)."""
import inspect
import json
import os
import sys
import types

import numpy as np
import pytest

from opensfm_amd import compat
from opensfm_amd.compat import pydense_full

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pydense_names.json")


def test_pruner_names_are_those_of_the_reference():
    names = json.load(open(GOLDEN))
    ours = {n for n, f in inspect.getmembers(pydense_full.DepthmapPruner, callable) if not n.startswith("_")}
    assert ours == set(names["DepthmapPruner"]), sorted(ours ^ set(names["DepthmapPruner"]))
    assert list(inspect.signature(pydense_full.DepthmapPruner.add_view).parameters) == ["self", "K", "R", "t", "depth", "plane", "color", "label"]
    assert list(inspect.signature(pydense_full.DepthmapPruner.set_same_depth_threshold).parameters) == ["self", "t"]
    # the two classes of compat.pydense, themselves; compat.pydense keeps its surface
    assert pydense_full.DepthmapEstimator is compat.pydense.DepthmapEstimator and pydense_full.DepthmapCleaner is compat.pydense.DepthmapCleaner
    assert not hasattr(compat.pydense, "DepthmapPruner") and not hasattr(pydense_full, "OpenMVSExporter")


def test_default_threshold_and_shape_messages():
    dp = pydense_full.DepthmapPruner()
    assert dp._params.same_depth_threshold == 0.01
    dp.set_same_depth_threshold(0.25)
    assert dp._params.same_depth_threshold == 0.25
    good = dict(depth=np.zeros((4, 5), np.float32), plane=np.zeros((4, 5, 3), np.float32), color=np.zeros((4, 5, 3), np.uint8),
                label=np.zeros((4, 5), np.uint8))
    for name, bad in (("plane", np.zeros((4, 6, 3), np.float32)), ("color", np.zeros((3, 5, 3), np.uint8)), ("label", np.zeros((5, 4), np.uint8))):
        with pytest.raises(ValueError, match=f"depth and {name} must have matching shapes."):
            dp.add_view(np.eye(3), np.eye(3), np.zeros(3), **{**good, name: bad})
    assert dp._views == []
    dp.add_view(np.eye(3), np.eye(3), np.zeros(3), **good)
    assert len(dp._views) == 1
    with pytest.raises(ValueError, match="no view was added"):
        pydense_full.DepthmapPruner().prune()


def _probe(name):
    pkg = types.ModuleType(name)
    sys.modules[name] = pkg
    return pkg


def _forget(name):
    for k in [k for k in sys.modules if k.startswith(name)]:
        del sys.modules[k]


def test_registration_as_pydense():
    pkg = _probe("osfm_full_probe")
    try:
        done = compat.install("osfm_full_probe", extra=("pydense_full",))
        assert sorted(done) == ["pybundle", "pydense", "pyfeatures", "pyrobust", "pysfm"] and "osfm_full_probe.pydense_full" not in sys.modules
        from osfm_full_probe import pydense

        assert pkg.pydense is pydense and pydense.DepthmapPruner is pydense_full.DepthmapPruner
        assert pydense.DepthmapEstimator is compat.pydense.DepthmapEstimator and pydense.DepthmapCleaner is compat.pydense.DepthmapCleaner
        with pytest.raises(AttributeError, match="OpenMVSExporter"):
            pydense.OpenMVSExporter
        for both in (("pydense", "pydense_full"), ("pydense_full", "pydense")):
            with pytest.raises(ValueError, match="not both"):
                compat.install("osfm_full_probe", extra=both)
        with pytest.raises(ValueError, match="pymap"):
            compat.install("osfm_full_probe", extra=("pymap",))
    finally:
        _forget("osfm_full_probe")
    _probe("osfm_full_probe2")
    try:
        done = compat.install_dense_full("osfm_full_probe2")
        assert sorted(done) == ["pybundle", "pydense", "pyfeatures", "pyrobust", "pysfm"]
        assert done["pydense"].DepthmapPruner is pydense_full.DepthmapPruner
    finally:
        _forget("osfm_full_probe2")


def test_install_and_install_dense_register_what_they_did():
    _probe("osfm_full_probe3")
    try:
        done = compat.install("osfm_full_probe3")
        assert sorted(done) == ["pybundle", "pyfeatures", "pyrobust", "pysfm"] and "osfm_full_probe3.pydense" not in sys.modules
    finally:
        _forget("osfm_full_probe3")
    _probe("osfm_full_probe4")
    try:
        done = compat.install_dense("osfm_full_probe4")
        assert sorted(done) == ["pybundle", "pydense", "pyfeatures", "pyrobust", "pysfm"]
        with pytest.raises(AttributeError, match="DepthmapPruner"):
            done["pydense"].DepthmapPruner
    finally:
        _forget("osfm_full_probe4")
    assert sorted(compat.MODULES) == ["pybundle", "pyfeatures", "pyrobust", "pysfm"]
    assert sorted(compat.EXTRA_MODULES) == ["pydense", "pydense_full"]
