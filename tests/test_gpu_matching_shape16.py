"""GPU parity of the integer store's fused matcher on the 16x16x64 MFMA shape (match16.hip), the default kernel, against its three
references, bit for bit in counts and rows: the 32x32x32 fused kernel (OSFM_MATCH_SWEEP_32X32), the exact VALU kernel
(OSFM_MATCH_EXACT_KERNEL) and the CPU oracle.  The cases sit where the new shape's maps differ from the old one's: image sizes
around the 16- and 32-row borders, duplicated descriptors in different 16-row groups of one class and in different classes, the
d^2 >= 2^22 range that is re-run exactly, pass B with 1 .. 33 candidates, and a list of pairs longer than the resident grid."""
import ctypes as C

import numpy as np
import pytest

from opensfm_amd import _lib, matching, synthetic

pytestmark = pytest.mark.gpu

KERNELS = {"sweep16": 0, "sweep32": _lib.MATCH_SWEEP_32X32, "exact": _lib.MATCH_EXACT_KERNEL}
MODES = {
    "symmetric": {},
    "one-way": {"symmetric_matching": False},
    "symmetric-squared": {"matcher_type": "FLANN"},
    "one-way-squared": {"symmetric_matching": False, "matcher_type": "FLANN"},
}


def _match(store, pairs, cfg, kernel, timings=None):
    lib = _lib.load()
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    prm = matching.make_params(cfg, robust=False)
    prm.flags |= KERNELS[kernel]
    res = C.c_void_p()
    _lib.check(lib.osfm_match_pairs(store.ctx.handle, store.handle, pairs.ctypes.data_as(C.POINTER(C.c_int32)), len(pairs), C.byref(prm),
                                    C.byref(res), C.byref(timings) if timings is not None else None), "osfm_match_pairs")
    counts, m = matching._fetch_result(lib, res)
    return np.array(counts, np.int32), np.array(m, np.int32).reshape(-1, 2)


def _oracle_pair(oracle_lib, mode, f1, f2, ratio):
    if len(f1) < 2 or len(f2) < 2:
        return np.zeros((0, 2), np.int32)
    if mode == "symmetric":
        return oracle_lib.match_brute_force_symmetric(f1, f2, ratio)
    if mode == "one-way":
        return oracle_lib.match_brute_force(f1, f2, ratio)
    if mode == "symmetric-squared":
        return oracle_lib.match_brute_force_symmetric(f1, f2, ratio, squared=True)
    return oracle_lib.match_flann(f1, f2, ratio)


def _check(oracle_lib, images, pairs, mode, ratio=0.8, oracle_pairs=None):
    """all three kernels on the pairs of one ragged store, and the oracle on oracle_pairs (default: every pair); returns the rows per pair"""
    cfg = dict(MODES[mode], lowes_ratio=ratio)
    store = matching.DescriptorStore(images, [np.zeros((len(f), 2)) for f in images])
    try:
        got = {k: _match(store, pairs, cfg, k) for k in KERNELS}
    finally:
        store.close()
    for k in ("sweep32", "exact"):
        assert np.array_equal(got["sweep16"][0], got[k][0]), (mode, k)
        assert np.array_equal(got["sweep16"][1], got[k][1]), (mode, k)
    rows = matching.split_matches(*got["sweep16"])
    for i in range(len(pairs)) if oracle_pairs is None else oracle_pairs:
        a, b = pairs[i]
        want = _oracle_pair(oracle_lib, mode, images[a], images[b], ratio)
        assert np.array_equal(rows[i], np.asarray(want, np.int32).reshape(-1, 2)), (mode, int(a), int(b))
    return rows


SIZES = [2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 272]


@pytest.mark.parametrize("mode", list(MODES))
def test_sizes_around_16_and_32_row_borders(oracle_lib, gpu_ctx, mode):
    """two images of every size (noisy subsets of one base set, so that re-examination, pass B and emission run); image A of size
    SIZES[i] against image B of sizes SIZES[i], SIZES[i + 3], SIZES[i + 7] (cyclically): each size meets small and large partners on
    both sides of the pair.  Plus (17, 300) and (300, 17)."""
    rng = np.random.default_rng(16)
    base = synthetic._hahog_like(rng, 300).astype(np.float32)

    def image(n):
        return np.clip(base[rng.permutation(300)[:n]] + np.rint(rng.normal(0, 3, (n, 128))), 0, 255).astype(np.float32)

    images = [image(n) for n in SIZES] + [image(n) for n in SIZES] + [image(17), image(300)]
    k = len(SIZES)
    pairs = [(i, k + (i + d) % k) for i in range(k) for d in (0, 3, 7)] + [(2 * k, 2 * k + 1), (2 * k + 1, 2 * k)]
    rows = _check(oracle_lib, images, np.array(pairs, np.int32), mode)
    assert sum(len(r) for r in rows) > 500


@pytest.mark.parametrize("ratio", [0.8, 1.0, 1.5])
def test_ties_within_a_class_and_across_classes(oracle_lib, gpu_ctx, ratio):
    """duplicated descriptors inside one image.  A class of the 16x16 sweep is the targets {64 k + 16 s + 8 h + j}: rows r and r + 16
    are two 16-row groups of one class (their maxima meet in the v_max3 tree), r and r + 8 the two halves of one wave's step (they
    meet in the chunk-end merge), r and r + 64 two waves.  Equal distances fail the strict ratio test below 1 and pass above it, and
    then the lowest index wins."""
    rng = np.random.default_rng(17)
    f1 = rng.integers(60, 196, (120, 128)).astype(np.float32)
    f2 = rng.integers(0, 30, (200, 128)).astype(np.float32)  # far background
    n_same = n_other = 0
    for i in range(90):
        r = (7 * i) % 100
        d = (16, 8, 64)[i % 3]
        if (f2[r] >= 60).any() or (f2[r + d] >= 60).any():
            continue  # the row already holds a planted copy
        f2[r] = f2[r + d] = np.clip(f1[i] + rng.integers(-2, 3, 128), 0, 255)
        n_same += d == 16
        n_other += d != 16
    assert n_same >= 10 and n_other >= 20
    for mode in ("symmetric", "one-way"):
        rows = _check(oracle_lib, [f1, f2], np.array([[0, 1], [1, 0]], np.int32), mode, ratio)
        if ratio > 1.0 and mode == "one-way":
            assert len(rows[0]) >= 30  # the duplicates do pass, with their lowest index


@pytest.mark.parametrize("ratio", [0.999, 1.5])
def test_extreme_range_is_flagged_and_rerun(oracle_lib, gpu_ctx, ratio):
    """all-0 rows against all-255 rows: d^2 = 128 * 255^2 = 8 323 200 >= 2^22, so the fused kernels flag the pair and the exact kernel
    decides it"""
    f1 = np.zeros((40, 128), np.float32)
    f2 = np.full((33, 128), 255, np.float32)
    from opensfm_amd._lib import MatchTimings

    store = matching.DescriptorStore([f1, f2], [np.zeros((40, 2)), np.zeros((33, 2))])
    tm = MatchTimings()
    _match(store, np.array([[0, 1]], np.int32), {"lowes_ratio": ratio}, "sweep16", tm)
    store.close()
    assert tm.pairs_exact_path == 1
    for mode in ("symmetric", "one-way"):
        _check(oracle_lib, [f1, f2], np.array([[0, 1], [1, 0]], np.int32), mode, ratio)


@pytest.mark.parametrize("k", [1, 15, 16, 17, 33])
def test_pass_b_with_k_candidates(oracle_lib, gpu_ctx, k):
    """k rows of the pair's first image are noisy copies of k rows of the second; everything else is unrelated, so pass A leaves k hits on k
    distinct features and pass B sweeps a gathered chunk of k queries (a partial step that enters at stage 7 or 6)"""
    rng = np.random.default_rng(100 + k)
    f1 = synthetic._hahog_like(rng, 150).astype(np.float32)
    f2 = synthetic._hahog_like(rng, 130).astype(np.float32)
    src = rng.permutation(130)[:k]
    dst = rng.permutation(150)[:k]
    f1[dst] = np.clip(f2[src] + rng.integers(-2, 3, (k, 128)), 0, 255)
    rows = _check(oracle_lib, [f1, f2], np.array([[0, 1]], np.int32), "symmetric")
    assert len(rows[0]) == k


def test_all_pairs_of_24_images(oracle_lib, gpu_ctx):
    """24 images x 2000 features through osfm_match_pairs: all 276 pairs against the three references, then the list thirty times
    over (8280 pairs): the call splits a list of 8192 pairs or more into two chunks, so two launches follow each other on one ticket
    buffer, and each has many more pairs than the resident grid has workgroups -- tickets, continued ranges, the hand-over between
    pairs and between chunks run with the new kernel, against the 32x32x32 kernel on the same list.  The oracle checks the pairs of
    the first image with its next neighbours and one far pair (a 2000 x 2000 pair takes the CPU about a second)."""
    from opensfm_amd._lib import MatchTimings

    sc = synthetic.make_matching_scene(24, 2000, seed=5)
    images = [sc.desc[sc.offsets[i]:sc.offsets[i + 1]].astype(np.float32) for i in range(24)]
    pairs = synthetic.all_pairs(24)
    rows = _check(oracle_lib, images, pairs, "symmetric", oracle_pairs=[0, 1, 2, 22])
    assert sum(len(r) > 0 for r in rows) >= 40 and sum(len(r) == 0 for r in rows) >= 40  # pairs with a tail and pairs that skip it
    reps = 30
    many = np.tile(pairs, (reps, 1))
    assert len(many) >= 8192
    store = matching.DescriptorStore(images, [np.zeros((2000, 2))] * 24)
    try:
        tm16, tm32 = MatchTimings(), MatchTimings()
        c16, m16 = _match(store, many, {}, "sweep16", tm16)
        c32, m32 = _match(store, many, {}, "sweep32", tm32)
    finally:
        store.close()
    assert tm16.match_launches >= 2 and tm32.match_launches >= 2
    assert np.array_equal(c16, c32) and np.array_equal(m16, m32)
    assert np.array_equal(c16, np.tile([len(r) for r in rows], reps))
    assert np.array_equal(m16, np.tile(np.concatenate(rows), (reps, 1)))
