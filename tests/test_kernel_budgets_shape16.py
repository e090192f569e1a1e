"""Budget of match_sweep16_kernel (opensfm_amd/csrc/match16.hip), the integer store's fused matcher on v_mfma_i32_16x16x64_i8,
checked without a GPU on the cross-compiled gfx950 assembly with the product's flags: two workgroups per CU, few spilled registers
and none of them touched inside the sweep, no static LDS (the kernel asks for the CU's whole dynamic LDS), 128 MFMAs per step, and
the longest run of vector / LDS / memory instructions between two MFMAs of a wave.  An MFMA of this shape holds the vector issue for
8 of its 16 cycles, so about two plain vector instructions hide behind each.  The walker is the one of
tests/test_kernel_budgets_sweep.py, for this kernel's MFMA and step marker."""
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

KERNEL = "match_sweep16_kernel"
MFMA = "v_mfma_i32_16x16x64_i8"
MARK = "#step"
# the values this build reaches (the build is deterministic).  Inside a full tile the longest gap between two MFMAs is 4 instructions (9
# and 13 in a step's first tile, which issues the next step's target fetch); the figures below are the walker's worst path, which runs
# through the stages a partial step skips (inside) and through the drain of the last tile's accumulators (26 instructions) into the
# next step's entry (across)
INSIDE_STEP = 56
ACROSS_BOUNDARY = 81


def kernel_body(asm):
    names = [m.group(1) for m in re.finditer(r"\n(_Z\w+):", asm) if KERNEL in m.group(1)]
    assert len(names) == 1, names
    a = asm.index("\n" + names[0] + ":")
    return names[0], asm[a: asm.index("s_endpgm", a)]


def blocks_of(text):
    """[(label, [instructions])] in program order: a block begins at a label and after every branch"""
    blocks = [("entry", [])]
    for ln in text.splitlines():
        if "osfm-step16" in ln:
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
            if k.startswith(("s_barrier", "s_endpgm")):
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


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("sweep16") / "match16.s"
    r = subprocess.run([HIPCC, *FLAGS, os.path.join(CSRC, "match16.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def _meta(asm, name, key):
    m = re.search(r"\.amdhsa_kernel %s\b[\s\S]*?\.end_amdhsa_kernel" % re.escape(name), asm)
    v = re.search(r"\.%s\s+(\d+)" % key, m.group(0))
    return int(v.group(1))


def test_registers_lds_and_scratch(asm):
    name, body = kernel_body(asm)
    assert not re.search(r"match_(fused|exact|float|hamming)_kernel", name)  # the 32x32x32 kernel's tests do not see this one
    info = asm[asm.index("s_endpgm", asm.index("\n" + name + ":")):]
    occupancy = int(re.search(r"; Occupancy: (\d+)", info).group(1))
    agprs = int(re.search(r"; NumAgprs: (\d+)", info).group(1))
    meta = asm[asm.index(".amdgpu_metadata"):]
    entry = meta[meta.index(".name:           " + name):]
    entry = entry[: entry.index(".wavefront_size")]
    spilled = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1))
    print("occupancy %d, AGPRs %d, spilled VGPRs %d" % (occupancy, agprs, spilled))
    assert occupancy == 2 and agprs == 0
    assert spilled <= 32
    assert _meta(asm, name, "amdhsa_group_segment_fixed_size") == 0
    blocks, _ = blocks_of(body)
    for label, ins in blocks:
        if any(k.startswith(MFMA) for k in ins):
            assert not any(k.startswith("scratch_") for k in ins), label
    assert not any(k.startswith("v_mfma") and not k.startswith(MFMA) for _, ins in blocks for k in ins)


def test_sweep_issue_runs_between_mfmas(asm):
    _, body = kernel_body(asm)
    blocks, index = blocks_of(body)
    first = next(i for i, (_, ins) in enumerate(blocks) if any(k.startswith(MFMA) for k in ins))
    last = next(i for i in range(first, len(blocks)) if any(k.startswith("s_barrier") for k in blocks[i][1]))
    # a full step: 8 query tiles x 16 MFMAs, between two step markers
    per_step, n = [], None
    for _, ins in blocks[first:last + 1]:
        for k in ins:
            if k == MARK:
                if n is not None:
                    per_step.append(n)
                n = 0
            elif n is not None and k.startswith(MFMA):
                n += 1
    print("MFMAs between step markers:", per_step)
    assert per_step and min(per_step) >= 128
    inside, across = longest_runs(blocks, index, first, last + 1)
    print("longest run inside a step: %d, across a step boundary: %d" % (inside, across))
    assert (inside, across) == (INSIDE_STEP, ACROSS_BOUNDARY)


def test_gaps_inside_a_full_tile(asm):
    """the figure that decides the sweep's speed: between two consecutive MFMAs of a fully unrolled query tile (a block of 16 MFMAs) at most
    4 vector / LDS / memory instructions in a plain tile -- an MFMA of this shape leaves room for about two, and a pair of gaps shares
    what one overruns -- and at most 13 in a step's first tile, which issues the next step's target fetch, and 7 in its last, which reads
    the next step's seeds"""
    _, body = kernel_body(asm)
    blocks, _ = blocks_of(body)
    gaps = []
    for _, ins in blocks:
        at = [i for i, k in enumerate(ins) if k.startswith(MFMA)]
        if len(at) == 16:
            gaps.append(max(sum(counted(k) for k in ins[a + 1:b]) for a, b in zip(at, at[1:])))
    print("largest gap per tile:", sorted(gaps))
    assert len(gaps) >= 16
    assert max(gaps) <= 13
    assert sum(g <= 4 for g in gaps) * 8 >= 6 * len(gaps)  # tiles 1 .. 6 of the 8 of every step
