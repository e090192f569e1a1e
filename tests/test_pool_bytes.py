"""OSFM_POOL_BYTES, the block cache a context may keep (opensfm_amd/csrc/osfm_internal.h), compiled for the host against tests/native/hipemu:
a plain decimal number of bytes is taken as it is; anything else -- empty, a sign, a suffix, a value past 2^64 - 1 -- falls back to the
default with one line on stderr instead of turning the cache off."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def build_host():
    src = os.path.join(HERE, "native", "pool_bytes_host.cpp")
    header = os.path.join(ROOT, "opensfm_amd", "csrc", "osfm_internal.h")
    out_dir = os.path.join(HERE, "native", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "pool_bytes_host.so")
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in (src, header)):
        subprocess.check_call([CLANG, "-O2", "-fPIC", "-shared", "-std=c++17", "-DOSFM_HIPEMU", "-I", os.path.join(HERE, "native", "hipemu"),
                               "-I", os.path.join(ROOT, "opensfm_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", so, src])
    lib = C.CDLL(so)
    lib.host_parse_pool_bytes.restype = C.c_int
    lib.host_parse_pool_bytes.argtypes = [C.c_char_p, C.POINTER(C.c_ulonglong)]
    lib.host_pool_limit_from_env.restype = C.c_ulonglong
    lib.host_default_pool_bytes.restype = C.c_ulonglong
    return lib


@pytest.fixture(scope="module")
def host():
    return build_host()


def parse(host, s):
    v = C.c_ulonglong(12345)
    ok = host.host_parse_pool_bytes(s.encode(), C.byref(v))
    return v.value if ok else None


@pytest.mark.parametrize("text, want", [("1073741824", 1 << 30), ("0", 0), ("18446744073709551615", 2**64 - 1)])
def test_plain_decimal_is_taken_as_it_is(host, text, want):
    assert parse(host, text) == want


@pytest.mark.parametrize("text", ["", "2G", "2e9", "-1", "+5", " 7", "7 ", "18446744073709551616", "99999999999999999999999"])
def test_anything_else_is_refused(host, text):
    assert parse(host, text) is None


def test_the_context_falls_back_to_the_default_with_a_warning(host, monkeypatch, capfd):
    default = host.host_default_pool_bytes()
    monkeypatch.delenv("OSFM_POOL_BYTES", raising=False)
    assert host.host_pool_limit_from_env() == default
    monkeypatch.setenv("OSFM_POOL_BYTES", "2147483648")
    assert host.host_pool_limit_from_env() == 2147483648
    assert capfd.readouterr().err == ""
    for bad in ("2G", "", "-1"):
        monkeypatch.setenv("OSFM_POOL_BYTES", bad)
        assert host.host_pool_limit_from_env() == default
        err = capfd.readouterr().err
        assert err.count("\n") == 1 and "OSFM_POOL_BYTES" in err, err
