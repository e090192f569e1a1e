"""The kernels' numerics and wavefront orchestration (host-compiled, tests/native/*.cpp) under AddressSanitizer +
UndefinedBehaviorSanitizer: an out-of-bounds index into an LDS-resident array or an uninitialised read is silent corruption on the
GPU; here it aborts the run."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_host_compiled_kernel_code_is_clean_under_asan_ubsan(oracle_lib):
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan is not available")
    out_dir = os.path.join(HERE, "native", "_build")
    os.makedirs(out_dir, exist_ok=True)
    sos = []
    for name in ("relpose_core_host", "guided_host"):
        so = os.path.join(out_dir, name + "_asan.so")
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-fPIC",
                               "-shared", "-std=c++17", "-o", so, os.path.join(HERE, "native", name + ".cpp")])
        sos.append(so)
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "native", "sanitizer_run.py")] + sos, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "relpose harness under ASan/UBSan: clean" in r.stdout and "guided harness under ASan/UBSan: clean" in r.stdout


def test_emulated_bundle_adjustment_is_clean_under_asan_ubsan(tmp_path):
    """The real bundle-adjustment sources (ba.hip, ba_generic.inc, the LM driver) on the host emulation, built with
    -fsanitize=address,undefined: two LM iterations of a [k1 k2 focal] scene, a local problem with constant cameras, a generic Brown scene
    and the rig / bias / control-point / up-vector scene of test_emu_ba.py.  This build found block_sum<3> of candidate_kernel's sixteen
    wavefronts writing 48 doubles into an LDS array of 32.  The process must end cleanly and walk the plain emulation's trajectory: both
    builds do the same IEEE operations (no contraction, no reassociation at either optimisation level), so the costs are the same bits.
    The sanitizer runtime is appended to whatever LD_PRELOAD the test inherits."""
    import emu_util

    build_emu = emu_util._builder()
    runtime = build_emu.asan_runtime()
    if runtime is None:
        pytest.skip("the compiler's shared AddressSanitizer runtime is not available")
    build_emu.build(sanitize=True)  # (cached by mtime, as the plain build; the child below finds it built)
    script = os.path.join(HERE, "native", "sanitizer_run_ba.py")
    spec = importlib.util.spec_from_file_location("sanitizer_run_ba", script)
    plain_run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(plain_run)
    plain_npz, asan_npz = str(tmp_path / "plain.npz"), str(tmp_path / "asan.npz")
    plain_run.main("plain", plain_npz)
    preload = " ".join(x for x in (os.environ.get("LD_PRELOAD", ""), runtime) if x)
    env = dict(os.environ, LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    r = subprocess.run([sys.executable, script, "asan", asan_npz], env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "emulated bundle adjustment (asan): clean" in r.stdout and "runtime error" not in r.stderr
    plain, asan = np.load(plain_npz), np.load(asan_npz)
    assert sorted(plain.files) == sorted(asan.files) and len(plain.files) == 4
    for name in plain.files:
        assert len(plain[name]) == 3 and np.array_equal(plain[name], asan[name]), (name, plain[name], asan[name])
