"""Builds tests/native/_build/libosfm_prune_emu.so: the product's depthmap pruning (opensfm_amd/csrc/prune.hip, unmodified) compiled for
the HOST against the HIP emulation of tests/native/hipemu, with the context plumbing of emu_ctx.cpp -- the three kernels and the host
side of the call then run on the CPU (depthmap.hip is linked beside it for ``osfm_depthmap_params_default``, which the Python layer
asks for its defaults).  ``build_main(name)`` links prune.hip and emu_ctx.cpp with tests/native/<name>.cpp (prune_main) into a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.  TEST INFRASTRUCTURE: nothing under opensfm_amd/ loads either."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "opensfm_amd", "csrc")
OUT = os.path.join(HERE, "_build")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FLAGS = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-DOSFM_HIPEMU", "-Wno-unknown-attributes", "-Wno-unused-value", "-Wno-pass-failed",
         "-I", os.path.join(HERE, "hipemu"), "-I", CSRC, "-I", os.path.join(ROOT, "include")]
SOURCES = ((os.path.join(CSRC, "prune.hip"), ["-x", "c++"]), (os.path.join(HERE, "emu_ctx.cpp"), []))
# the shared library alone: osfm_depthmap_params_default lives in depthmap.hip, and the Python layer asks it for its defaults
LIB_SOURCES = SOURCES + ((os.path.join(CSRC, "depthmap.hip"), ["-x", "c++"]),)


def _deps():
    deps = [src for src, _ in LIB_SOURCES] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    deps += [os.path.abspath(__file__), os.path.join(ROOT, "include", "osfm_mi355.h")]
    return deps + [os.path.join(dp, f) for dp, _, fs in os.walk(os.path.join(HERE, "hipemu")) for f in fs]


def _fresh(target, deps):
    return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in deps)


def _objects(prefix, extra, sources=SOURCES):
    objs = []
    for src, lang in sources:
        o = os.path.join(OUT, prefix + os.path.basename(src).split(".")[0] + ".o")
        subprocess.check_call([CLANG] + FLAGS + extra + lang + ["-c", src, "-o", o])
        objs.append(o)
    return objs


def build(force: bool = False) -> str:
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, "libosfm_prune_emu.so")
    if not force and _fresh(so, _deps()):
        return so
    subprocess.check_call([CLANG, "-shared", "-fPIC"] + _objects("prune_emu_", [], LIB_SOURCES) + ["-o", so, "-lpthread"])
    return so


def build_main(name: str = "prune_main", force: bool = False) -> str:
    """the stand-alone sanitised program of tests/native/<name>.cpp (its own main; nothing of it is loaded into Python)"""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name + "_asan")
    main = os.path.join(HERE, name + ".cpp")
    if not force and _fresh(exe, _deps() + [main]):
        return exe
    # (a fibre's whole stack shadow is cleared at every switch to it: small stacks keep the run short)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-DHIPEMU_STACK_BYTES=131072"]
    objs = _objects("prune_asan_", san)
    subprocess.check_call([CLANG] + FLAGS + san + [main] + objs + ["-o", exe, "-lpthread"])
    return exe


if __name__ == "__main__":
    print(build(force=True))
    print(build_main("prune_main", force=True))
