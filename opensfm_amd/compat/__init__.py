"""Modules under the names of the reference's pybind11 extensions -- ``pyfeatures``, ``pyrobust``, ``pybundle``, ``pysfm`` -- holding the
entries of their surfaces that lie on the hot path (``opensfm/src/*/python/pybind.cc``), served by ``libosfm_mi355.so``.

The reference imports its extensions as ``from opensfm import pyfeatures`` ...; a deployment that wants ``bin/opensfm_run_all`` untouched
puts these modules in front: ``opensfm_amd.compat.install()`` registers them in ``sys.modules`` as ``opensfm.pyfeatures`` etc. for every
name that is NOT already importable (it never shadows a compiled extension unless ``force=True``), attribute by attribute: an attribute
this package does not provide is looked up in the compiled module when there is one, and raises ``AttributeError`` naming the missing
entry otherwise -- there is no CPU fallback behind these names.

``pydense`` (``DepthmapEstimator``, ``DepthmapCleaner``) is registered on request only: ``install(..., extra=("pydense",))`` or
``install_dense()``; what ``install()`` registers by default does not change.  ``pydense_full`` is ``pydense`` plus ``DepthmapPruner``:
``install(..., extra=("pydense_full",))`` or ``install_dense_full()`` registers it AS ``<package>.pydense`` (asking for both is a
``ValueError``)."""
import importlib
import sys
import types
from typing import Dict, Sequence

from . import pybundle, pydense, pydense_full, pyfeatures, pyrobust, pysfm

MODULES = {"pyfeatures": pyfeatures, "pyrobust": pyrobust, "pybundle": pybundle, "pysfm": pysfm}
EXTRA_MODULES = {"pydense": pydense, "pydense_full": pydense_full}  # registered only when asked for
REGISTERED_AS = {"pydense_full": "pydense"}  # an optional module that goes under another's name


class _Overlay(types.ModuleType):
    """attributes of the GPU module first, then of the compiled module it stands in front of"""

    def __init__(self, name: str, gpu, compiled=None):
        super().__init__(name, gpu.__doc__)
        self.__dict__["_gpu"], self.__dict__["_compiled"] = gpu, compiled

    def __getattr__(self, attr):
        for m in (self.__dict__["_gpu"], self.__dict__["_compiled"]):
            if m is not None and hasattr(m, attr):
                return getattr(m, attr)
        raise AttributeError(f"{self.__name__}.{attr} is not provided by opensfm_amd.compat (GPU hot-path subset) and no compiled module is present")


def install(package: str = "opensfm", force: bool = False, extra: Sequence[str] = ()) -> Dict[str, types.ModuleType]:
    """register ``<package>.pyfeatures`` ... in ``sys.modules``, and the modules of EXTRA_MODULES named in `extra`; returns what was
    registered, by the name it was registered under (``pydense_full`` goes under ``pydense``)"""
    done = {}
    wanted = dict(MODULES)
    for name in extra:
        if name not in EXTRA_MODULES:
            raise ValueError(f"opensfm_amd.compat has no optional module {name!r} (there is: {sorted(EXTRA_MODULES)})")
        target = REGISTERED_AS.get(name, name)
        if target in wanted and wanted[target] is not EXTRA_MODULES[name]:
            raise ValueError(f"opensfm_amd.compat: {name!r} is registered as {target!r}: ask for one of them, not both")
        wanted[target] = EXTRA_MODULES[name]
    for name, gpu in wanted.items():
        full = f"{package}.{name}"
        compiled = None
        try:
            compiled = importlib.import_module(full)
            if isinstance(compiled, _Overlay):  # installed before
                if not force:
                    continue
                compiled = compiled.__dict__["_compiled"]
        except Exception:  # noqa: BLE001 -- the compiled extension is absent (or its own imports fail)
            compiled = None
        if compiled is not None and not force:
            continue
        sys.modules[full] = done[name] = _Overlay(full, gpu, compiled)
        pkg = sys.modules.get(package)
        if pkg is not None:
            setattr(pkg, name, done[name])
    return done


def install_dense(package: str = "opensfm", force: bool = False) -> Dict[str, types.ModuleType]:
    """``install(package, force, extra=("pydense",))``: the default modules and ``<package>.pydense``"""
    return install(package, force, extra=("pydense",))


def install_dense_full(package: str = "opensfm", force: bool = False) -> Dict[str, types.ModuleType]:
    """``install(package, force, extra=("pydense_full",))``: the default modules and ``<package>.pydense`` with ``DepthmapPruner``"""
    return install(package, force, extra=("pydense_full",))
