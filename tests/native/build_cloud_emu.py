"""Builds tests/native/_build/libosfm_cloud_emu.so: the product's point-cloud filters (opensfm_amd/csrc/cloud.hip, unmodified) compiled for
the HOST against the HIP emulation of tests/native/hipemu, with the context plumbing of emu_ctx.cpp -- both kernels of each filter and the
host side of the library then run on the CPU.  TEST INFRASTRUCTURE: nothing under opensfm_amd/ loads this library."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "opensfm_amd", "csrc")
OUT = os.path.join(HERE, "_build")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def build(force: bool = False) -> str:
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, "libosfm_cloud_emu.so")
    deps = [os.path.join(CSRC, "cloud.hip")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    deps += [os.path.join(HERE, "emu_ctx.cpp"), os.path.abspath(__file__)]
    deps += [os.path.join(dp, f) for dp, _, fs in os.walk(os.path.join(HERE, "hipemu")) for f in fs]
    deps.append(os.path.join(ROOT, "include", "osfm_mi355.h"))
    if not force and os.path.exists(so) and all(os.path.getmtime(so) >= os.path.getmtime(d) for d in deps):
        return so
    flags = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-DOSFM_HIPEMU", "-Wno-unknown-attributes", "-Wno-unused-value", "-Wno-pass-failed",
             "-I", os.path.join(HERE, "hipemu"), "-I", CSRC, "-I", os.path.join(ROOT, "include")]
    objs = []
    for src, lang in ((os.path.join(CSRC, "cloud.hip"), ["-x", "c++"]), (os.path.join(HERE, "emu_ctx.cpp"), [])):
        o = os.path.join(OUT, "cloud_emu_" + os.path.basename(src).split(".")[0] + ".o")
        subprocess.check_call([CLANG] + flags + lang + ["-c", src, "-o", o])
        objs.append(o)
    subprocess.check_call([CLANG, "-shared", "-fPIC"] + objs + ["-o", so, "-lpthread"])
    return so


if __name__ == "__main__":
    print(build(force=True))
