"""``pydense`` with the pruner: ``DepthmapEstimator`` and ``DepthmapCleaner`` of ``compat.pydense`` and ``DepthmapPruner`` with the
wrapper's method names and argument order (``depthmap_bind.h``), served by ``osfm_depthmap_prune``.  ``compat.pydense`` keeps its
surface; this module is registered in its place, as ``<package>.pydense``, by ``install(extra=("pydense_full",))`` or
``install_dense_full()``.  ``OpenMVSExporter`` (file writing) is not provided: the overlay's ``AttributeError`` names it."""
import numpy as np

from .. import dense as _dense
from .pydense import DepthmapCleaner, DepthmapEstimator, _view

__all__ = ["DepthmapEstimator", "DepthmapCleaner", "DepthmapPruner"]


class DepthmapPruner:
    def __init__(self):
        self._params = _dense.default_params()
        self._params.same_depth_threshold = 0.01  # DepthmapPruner's own default
        self._views = []

    def set_same_depth_threshold(self, t):
        self._params.same_depth_threshold = float(t)

    def add_view(self, K, R, t, depth, plane, color, label):
        depth, plane, color, label = np.asarray(depth), np.asarray(plane), np.asarray(color), np.asarray(label)
        if depth.ndim != 2:
            raise ValueError("depth must be a (height, width) array")
        for name, a in (("plane", plane), ("color", color), ("label", label)):
            if a.shape[:2] != depth.shape:
                raise ValueError(f"depth and {name} must have matching shapes.")
        self._views.append(_view(K, R, t) + (np.ascontiguousarray(depth, np.float32), np.ascontiguousarray(plane, np.float32),
                                             np.ascontiguousarray(color, np.uint8), np.ascontiguousarray(label, np.uint8)))

    def prune(self):
        """[points (n, 3) float32, normals (n, 3) float32, colors (n, 3) uint8, labels (n,) uint8] of the first view added"""
        if not self._views:
            raise ValueError("no view was added")
        return list(_dense.prune_raw([{"views": self._views}], self._params)[0])
