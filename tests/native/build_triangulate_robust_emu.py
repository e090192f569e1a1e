"""Builds tests/native/_build/libosfm_triangulate_robust_emu.so: opensfm_amd/csrc/triangulate.hip (unmodified, the robust kernels and
triangulate_robust.h included) compiled for the HOST against the HIP emulation of tests/native/hipemu, as build_triangulate_emu.py does
for the FULL path -- its flags, sources and helpers are used as they are; this builder has its own output names and a dependency list
that knows the robust header.  ``build_main()`` links the same sources with tests/native/triangulate_robust_main.cpp into a stand-alone
program under AddressSanitizer and UndefinedBehaviorSanitizer.  TEST INFRASTRUCTURE: nothing under opensfm_amd/ loads either."""
import importlib.util
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def _full():
    spec = importlib.util.spec_from_file_location("build_triangulate_emu", os.path.join(HERE, "build_triangulate_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


full = _full()
OUT = full.OUT


def _deps():
    return full._deps() + [os.path.join(full.CSRC, "triangulate_robust.h"), os.path.abspath(__file__)]


def build(force: bool = False) -> str:
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, "libosfm_triangulate_robust_emu.so")
    if not force and full._fresh(so, _deps()):
        return so
    subprocess.check_call([full.CLANG, "-shared", "-fPIC"] + full._objects("triangulate_robust_emu_", []) + ["-o", so, "-lpthread"])
    return so


def build_main(force: bool = False) -> str:
    """the stand-alone sanitised program (its own main; nothing of it is loaded into Python)"""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "triangulate_robust_main_asan")
    main = os.path.join(HERE, "triangulate_robust_main.cpp")
    if not force and full._fresh(exe, _deps() + [main]):
        return exe
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-DHIPEMU_STACK_BYTES=131072"]
    objs = full._objects("triangulate_robust_asan_", san)
    subprocess.check_call([full.CLANG] + full.FLAGS + san + [main] + objs + ["-o", exe, "-lpthread"])
    return exe


if __name__ == "__main__":
    print(build(force=True))
    print(build_main(force=True))
