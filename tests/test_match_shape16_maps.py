"""The index maps of the matcher's 16x16x64 sweep (opensfm_amd/csrc/match16_maps.h), compiled for the host and checked without a GPU:
which target an accumulator register holds, which targets make up a class, the ordinal that carries cv2's lowest-index rule through
the class re-examination, and the lane addresses of a 16 x 64 operand fragment in the store's tile layout."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opensfm_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

SHIM = r"""
#include "match16_maps.h"
static_assert(osfm16_class_of_target(osfm16_target(3, 2, 1, 2, 3)) == osfm16_class_id(3, 2, 1), "constexpr");
extern "C" {
int frag_offset(int sub, int h, int lane) { return osfm16_frag_offset(sub, h, lane); }
int frag_row(int sub, int lane) { return osfm16_frag_row(sub, lane); }
int frag_piece(int h, int lane) { return osfm16_frag_piece(h, lane); }
int target(int rb, int w, int g, int s, int r) { return osfm16_target(rb, w, g, s, r); }
int class_id(int rb, int w, int g) { return osfm16_class_id(rb, w, g); }
int class_of_target(int t) { return osfm16_class_of_target(t); }
int class_target(int id, int ordinal) { return osfm16_class_target(id, ordinal); }
int ordinal(int t) { return osfm16_ordinal(t); }
}
"""


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    d = tmp_path_factory.mktemp("maps16")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return C.CDLL(str(so))


@pytest.mark.parametrize("tT", [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65])
def test_registers_cover_every_target_once(maps, tT):
    """(step, wave, lane group, sub-tile, register) -> target is injective, and the steps of an image of tT row tiles cover all of
    its 32 tT rows (a step covers 8 row tiles; what lies beyond the image is the slack the kernel pads with)"""
    nrb = (tT + 7) // 8
    seen = {}
    for rb in range(nrb):
        for w in range(4):
            for g in range(4):
                for s in range(4):
                    for r in range(4):
                        t = maps.target(rb, w, g, s, r)
                        assert t not in seen, (t, seen[t], (rb, w, g, s, r))
                        seen[t] = (rb, w, g, s, r)
                        # the wave's row tiles are 8 rb + 2 w and the next one, sub-tile s is 16 rows of them
                        assert t // 32 == rb * 8 + w * 2 + s // 2 and t % 32 == 16 * (s % 2) + 4 * g + r
    assert set(range(32 * tT)) <= set(seen)
    assert len(seen) == nrb * 256 and max(seen) < nrb * 256


def test_class_maps_agree(maps):
    n_classes = 9 * 8
    members = {}
    for rb in range(9):
        for w in range(4):
            for g in range(4):
                cid = maps.class_id(rb, w, g)
                assert cid == rb * 8 + w * 2 + g // 2  # the id packed into the chunk-end merge: row block * 8 + part
                for s in range(4):
                    for r in range(4):
                        t = maps.target(rb, w, g, s, r)
                        assert maps.class_of_target(t) == cid
                        members.setdefault(cid, []).append(t)
    assert len(members) == n_classes
    for cid, ts in members.items():
        assert len(ts) == 32 and len(set(ts)) == 32
        # class id -> target set, and its inverse
        assert sorted(ts) == [maps.class_target(cid, o) for o in range(32)]
        for o in range(32):
            assert maps.ordinal(maps.class_target(cid, o)) == o
        # the re-examination gives lane sl the ordinals sl and 16 + sl: 32 rows apart
        for sl in range(16):
            assert maps.class_target(cid, 16 + sl) == maps.class_target(cid, sl) + 32


def test_ordinal_order_is_ascending_target_index(maps):
    for cid in (0, 1, 6, 7, 8, 71):
        ts = [maps.class_target(cid, o) for o in range(32)]
        assert ts == sorted(ts) and len(set(ts)) == 32


def test_lane_addresses_reproduce_the_operand(maps):
    """a tile filled with its own byte offsets: element j of lane l's 16-byte fragment must be the byte of row 16 sub + (l & 15),
    dimension 64 h + 16 (l >> 4) + j, which the store keeps at piece * 512 + row * 16 + j"""
    tile = np.arange(4096, dtype=np.int64)
    for sub in range(2):
        for h in range(2):
            operand = np.full((16, 64), -1, np.int64)
            for lane in range(64):
                off = maps.frag_offset(sub, h, lane)
                assert off % 16 == 0 and 0 <= off <= 4096 - 16
                frag = tile[off:off + 16]
                operand[lane & 15, 16 * (lane >> 4):16 * (lane >> 4) + 16] = frag
                assert maps.frag_row(sub, lane) == 16 * sub + (lane & 15) and maps.frag_piece(h, lane) == 4 * h + (lane >> 4)
            for row in range(16):
                for k in range(64):
                    dim = 64 * h + k
                    assert operand[row, k] == (dim // 16) * 512 + (16 * sub + row) * 16 + dim % 16
            # 16 consecutive lanes read 256 contiguous bytes
            for g in range(4):
                offs = [maps.frag_offset(sub, h, 16 * g + i) for i in range(16)]
                assert offs == list(range(offs[0], offs[0] + 256, 16))
