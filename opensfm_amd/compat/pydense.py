"""``pydense`` (``opensfm/src/dense/python/pybind.cc``): ``DepthmapEstimator`` and ``DepthmapCleaner`` with the wrapper's method names and
argument order (``depthmap_bind.h``), served by ``osfm_depthmap_estimate`` / ``osfm_depthmap_clean``.  ``DepthmapPruner`` is not part of
this module's surface (``compat.pydense_full`` adds it) and ``OpenMVSExporter`` (file writing) is not provided: the overlay's
``AttributeError`` names them.

One addition: a ``seed`` property.  The reference seeds itself from ``random_device``; here a run is reproducible, and the default seed
is fixed."""
import numpy as np

from .. import dense as _dense


def _view(K, R, t):
    return np.asarray(K, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)


class DepthmapEstimator:
    def __init__(self):
        self._params = _dense.default_params()
        self._params.num_depth_planes = 50  # DepthmapEstimator's own default
        self._params.min_patch_sd = 5.0
        self._views = []
        self._seed = _dense.DEFAULT_SEED

    @property
    def seed(self):
        """the seed of every random draw of this estimator's PatchMatch runs (fixed by default: a run is reproducible)"""
        return self._seed

    @seed.setter
    def seed(self, value):
        self._seed = int(value)

    def set_depth_range(self, min_depth, max_depth, num_depth_planes):
        self._params.min_depth, self._params.max_depth = float(min_depth), float(max_depth)
        self._params.num_depth_planes = int(num_depth_planes)

    def set_patchmatch_iterations(self, n):
        self._params.patchmatch_iterations = int(n)

    def set_patch_size(self, size):
        self._params.patch_size = int(size)

    def set_min_patch_sd(self, sd):
        self._params.min_patch_sd = float(sd)

    def add_view(self, K, R, t, image, mask):
        image, mask = np.asarray(image), np.asarray(mask)
        if image.ndim != 2 or image.shape != mask.shape:
            raise ValueError("image and mask must have matching shapes.")
        self._views.append(_view(K, R, t) + (np.ascontiguousarray(image, np.uint8), np.ascontiguousarray(mask, np.uint8)))

    def _compute(self, method):
        if not self._views:
            raise ValueError("no view was added")
        self._params.method = _dense.METHODS[method]
        problem = {"views": self._views, "min_depth": self._params.min_depth, "max_depth": self._params.max_depth}
        (depth, plane, score, nghbr), = _dense.estimate_raw([problem], self._params, self.seed)[0]
        return [depth, plane, score, nghbr]

    def compute_patch_match(self):
        return self._compute("PATCH_MATCH")

    def compute_patch_match_sample(self):
        return self._compute("PATCH_MATCH_SAMPLE")

    def compute_brute_force(self):
        return self._compute("BRUTE_FORCE")


class DepthmapCleaner:
    def __init__(self):
        self._params = _dense.default_params()
        self._params.same_depth_threshold = 0.01
        self._params.min_consistent_views = 2  # DepthmapCleaner's own default
        self._views = []

    def set_same_depth_threshold(self, t):
        self._params.same_depth_threshold = float(t)

    def set_min_consistent_views(self, n):
        self._params.min_consistent_views = int(n)

    def add_view(self, K, R, t, depth):
        depth = np.asarray(depth)
        if depth.ndim != 2:
            raise ValueError("depth must be a (height, width) array")
        self._views.append(_view(K, R, t) + (np.ascontiguousarray(depth, np.float32),))

    def clean(self):
        if not self._views:
            raise ValueError("no view was added")
        return _dense.clean_raw([{"views": self._views}], self._params)[0][0]
