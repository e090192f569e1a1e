"""The resident grid of the fused matcher, checked without a GPU on the cross-compiled gfx950 assembly (flags and parsing of
tests/test_kernel_budgets.py): both instantiations of match_fused_kernel draw their pairs by ticket inside the kernel -- a global
atomic add ahead of the first MFMA, and more of them for the later pairs -- and loop over them -- a branch behind the last MFMA of the passes back to a label ahead of the
first one -- and the loop has brought no static LDS with it (the kernel asks for its LDS dynamically, up to the CU's whole 160 KiB)."""
import re

import pytest

from test_kernel_budgets import HIPCC, body, compile_device, one

pytestmark = pytest.mark.skipif(not __import__("os").path.exists(HIPCC), reason="hipcc not installed")

MFMA = "v_mfma_i32_32x32x32_i8"


@pytest.mark.parametrize("fq", ["ILb0E", "ILb1E"])  # integer store / float store
def test_fused_kernel_loops_over_tickets(tmp_path_factory, fq):
    asm, k = compile_device("match", tmp_path_factory)
    r, name = one(k, "match_fused_kernel", fq)
    assert r["LDS Size"] == 0, r
    lines = [ln.split(";")[0].strip() for ln in body(asm, name).splitlines()]
    lines = [ln for ln in lines if ln]
    mfmas = [i for i, ln in enumerate(lines) if ln.startswith(MFMA)]
    labels = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"(\.LBB\d+_\d+):", ln)] if m}
    atomics = [i for i, ln in enumerate(lines) if ln.startswith("global_atomic_add")]
    assert atomics and atomics[0] < mfmas[0], atomics  # the first ticket is drawn before any pass
    assert len(atomics) >= 2, atomics  # and the later ones inside the loop (where the compiler lays that block out is its business)
    back = [i for i, ln in enumerate(lines) if ln.startswith(("s_branch", "s_cbranch")) and i > mfmas[-1] and labels.get(ln.split()[1], i) < mfmas[0]]
    assert back, "no branch from behind the passes back to ahead of them"
