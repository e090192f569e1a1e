"""Issue runs of the matcher's sweep, checked without a GPU on the cross-compiled gfx950 assembly (same flags and parsing as
tests/test_kernel_budgets.py).  An in-order wavefront hides about five plain instructions behind a 32-cycle MFMA; a longer run of
vector-ALU / LDS / vector-memory instructions between two consecutive MFMAs of a wave is time in which only the partner wave keeps the
matrix pipe busy.  For pass A of match_fused_kernel<false> (the blocks from its first MFMA to the barrier that ends the sweep) this
test follows every path of the control-flow graph from an MFMA to the next one, the loop's back edge included, through the blocks of
the FULL step: a path ends at a barrier, and does not enter a block that fetches targets without issuing MFMAs (the fetch a partial
step, or a wave without targets, issues ahead of itself).  The longest run of two
kinds is taken: inside a step, and across a step boundary (the run passes the marker comment the kernel leaves where a step begins).
On the parent of the change that added this test the longest run was 39 inside the step (the eight class-index selects of a step, sunk
into its last tile, next to the nine LDS reads of the seeds) and 24 + about 55 across the boundary (the drain; then the seed moves and
the address arithmetic and issue of the target fetch, which now ride in the gaps of the step's first tile)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opensfm_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only"]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

MFMA = "v_mfma_i32_32x32x32_i8"
MARK = "#step"
INSIDE_STEP = 14      # the values this build reaches (the build is deterministic)
ACROSS_BOUNDARY = 25


def kernel_body(asm, *parts):
    names = [m.group(1) for m in re.finditer(r"\n(_Z\w+):", asm) if all(p in m.group(1) for p in parts)]
    assert len(names) == 1, names
    a = asm.index("\n" + names[0] + ":")
    return asm[a: asm.index("s_endpgm", a)]


def blocks_of(text):
    """[(label, [instructions])] in program order: a block begins at a label and after every branch"""
    blocks = [("entry", [])]
    for ln in text.splitlines():
        if "osfm-step" in ln:
            blocks[-1][1].append(MARK)
            continue
        ln = ln.split(";")[0].strip()
        m = re.match(r"(\.LBB\d+_\d+):", ln)
        if m:
            blocks.append((m.group(1), []))
        elif ln and not ln.startswith(".") and not re.match(r"[\w$.]+:", ln):
            blocks[-1][1].append(ln)
            if ln.startswith(("s_cbranch", "s_branch")):
                blocks.append(("after " + blocks[-1][0] + "/%d" % len(blocks), []))
    return blocks, {lab: i for i, (lab, _) in enumerate(blocks)}


def counted(ins):
    return ins.startswith(("v_", "ds_", "global_", "buffer_", "flat_", "scratch_")) and not ins.startswith(MFMA)


def ends_run(ins):
    return ins.startswith("s_barrier") or ins.startswith("s_endpgm")


def longest_runs(blocks, index, first, last):
    """longest (inside a step, across a step boundary) run over every path MFMA -> next MFMA that starts in blocks[first:last]"""
    best = [0, 0]
    fetch_only = [any(k.startswith("global_load") for k in ins) and not any(k.startswith(MFMA) for k in ins) for _, ins in blocks]

    def walk(b, i, n, crossed, seen):
        if b >= len(blocks) or b in seen or fetch_only[b]:
            return
        seen = seen | {b}
        for k in blocks[b][1][i:]:
            if k.startswith(MFMA):
                best[crossed] = max(best[crossed], n)
                return
            if ends_run(k):
                return
            if k == MARK:
                crossed = 1
            n += counted(k)
            if k.startswith("s_cbranch"):
                walk(index[k.split()[1]], 0, n, crossed, seen)
            if k.startswith("s_branch"):
                return walk(index[k.split()[1]], 0, n, crossed, seen)
        walk(b + 1, 0, n, crossed, seen)

    for b in range(first, last):
        for i, k in enumerate(blocks[b][1]):
            if k.startswith(MFMA):
                walk(b, i + 1, 0, 0, frozenset())
    return tuple(best)


def sweep_runs(asm):
    blocks, index = blocks_of(kernel_body(asm, "match_fused_kernel", "ILb0E"))
    first = next(i for i, (_, ins) in enumerate(blocks) if any(k.startswith(MFMA) for k in ins))
    last = next(i for i in range(first, len(blocks)) if any(k.startswith("s_barrier") for k in blocks[i][1]))
    assert sum(k.startswith(MFMA) for _, ins in blocks[first:last + 1] for k in ins) >= 64
    return longest_runs(blocks, index, first, last + 1)


@pytest.fixture(scope="module")
def match_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("sweep") / "match.s"
    r = subprocess.run([HIPCC, *FLAGS, os.path.join(CSRC, "match.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def test_sweep_issue_runs_between_mfmas(match_asm):
    """parent: 39 inside the step, 24 + about 55 across the step boundary; both must stay below that"""
    inside, across = sweep_runs(match_asm)
    print("longest run inside a step: %d, across a step boundary: %d" % (inside, across))
    assert inside < 39 and across < 24 + 55
    assert (inside, across) == (INSIDE_STEP, ACROSS_BOUNDARY)


def test_matcher_kernels_have_no_static_lds(match_asm):
    """osfm_match_init raises every matcher kernel's dynamic LDS limit to the CU's whole 160 KiB; the runtime refuses that for a
    kernel that also has static LDS (a library workgroup reduction such as __syncthreads_or brings 256 bytes of its own)"""
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.amdhsa_kernel (\w+)[\s\S]*?\.amdhsa_group_segment_fixed_size (\d+)", match_asm)}
    matchers = {k: v for k, v in sizes.items() if re.search(r"match_(fused|exact|float|hamming)_kernel", k)}
    assert len(matchers) == 5, sizes
    assert all(v == 0 for v in matchers.values()), matchers
