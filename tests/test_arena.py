"""OsfmArena, the one block a batched call carves its device buffers from (opensfm_amd/csrc/osfm_internal.h), compiled for the host
against tests/native/hipemu: tests/native/arena_main.cpp, a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer,
checks the byte total, the alignment, the bounds and the disjointness of the buffers for size lists with 0, 1, 255, 256 and 257 bytes
and a zero in first, middle and last position, and that a second arena of the same shape gets the cached block back."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def build_main():
    native = os.path.join(HERE, "native")
    sources = [os.path.join(native, "arena_main.cpp"), os.path.join(native, "emu_ctx.cpp")]
    deps = sources + [os.path.join(ROOT, "opensfm_amd", "csrc", "osfm_internal.h"), os.path.join(ROOT, "include", "osfm_mi355.h"), os.path.abspath(__file__)]
    deps += [os.path.join(dp, f) for dp, _, fs in os.walk(os.path.join(native, "hipemu")) for f in fs]
    out_dir = os.path.join(native, "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "arena_main_asan")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-DOSFM_HIPEMU", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-fno-omit-frame-pointer", "-I", os.path.join(native, "hipemu"), "-I", os.path.join(ROOT, "opensfm_amd", "csrc"),
                               "-I", os.path.join(ROOT, "include")] + sources + ["-o", exe, "-lpthread"])
    return exe


def test_arena_buffers_are_aligned_disjoint_inside_the_block_and_the_block_is_reused():
    run = subprocess.run([build_main()], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("OK 7 lists"), run.stdout
