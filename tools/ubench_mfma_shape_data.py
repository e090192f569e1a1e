"""Operands for tools/ubench_mfma_shape: two images of the bench scene, signed (a - 128), in the store's tile layout.

File: int32 nQ, int32 nT, then ceil(nQ / 32) query tiles and ceil(nT / 32) target tiles of 4096 bytes; piece q (16
dimensions) of row r sits at q * 512 + r * 16 of its tile, rows beyond the image are zero.
"""
import sys

import numpy as np

from opensfm_amd import synthetic


def tiles(desc: np.ndarray) -> np.ndarray:
    n = len(desc)
    t = (n + 31) // 32
    pad = np.zeros((t * 32, 128), np.int8)
    pad[:n] = (desc.astype(np.int16) - 128).astype(np.int8)
    # [tile][row][piece][16] -> [tile][piece][row][16]
    return np.ascontiguousarray(pad.reshape(t, 32, 8, 16).transpose(0, 2, 1, 3))


def main() -> None:
    out = sys.argv[1]
    scene = synthetic.make_matching_scene(1000, 2000, seed=42)
    q, _ = scene.image(1)
    t, _ = scene.image(0)
    with open(out, "wb") as f:
        np.array([len(q), len(t)], np.int32).tofile(f)
        tiles(q).tofile(f)
        tiles(t).tofile(f)
    print(f"{out}: {len(q)} queries, {len(t)} targets")


if __name__ == "__main__":
    main()
