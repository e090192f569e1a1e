"""GPU parity of the fused matcher at the sizes where its sweep changes shape: partial steps (a chunk with fewer than 8 query tiles
enters the tile sequence late), row blocks in which only some waves have targets, the odd last step of a chunk, the carry of the
per-class state over several chunks, and the tail that an empty pair skips (no candidate list, no pass B, no emission scan).  Every
case is compared exactly against the CPU oracle, through the leaf functions and through the batched entry point."""
import numpy as np
import pytest

from opensfm_amd import matching, synthetic

pytestmark = pytest.mark.gpu


def _tuples(m):
    return [tuple(int(v) for v in x) for x in m]


def _pair(n1, n2, seed):
    """two HAHOG-like images with min(n1, n2) // 2 planted noisy copies: re-examination, pass B and emission all run"""
    rng = np.random.default_rng(seed)
    f1 = synthetic._hahog_like(rng, n1).astype(np.float32)
    f2 = synthetic._hahog_like(rng, n2).astype(np.float32)
    k = min(n1, n2) // 2
    f2[:k] = np.clip(f1[rng.permutation(n1)[:k]] + np.rint(rng.normal(0, 3, (k, 128))), 0, 255)
    return f1, f2


def _both_orders(sizes):
    out = []
    for a, b in sizes:
        for s in ((a, b), (b, a)):
            if s not in out:
                out.append(s)
    return out


TILE_EDGES = [(n, m) for n in (2, 31, 32, 33) for m in (33, 300)]
QUERY_TILES = [(n, 300) for n in (224, 225, 256, 257)]          # 7 vs 8 query tiles in a chunk; 1 vs 2 chunks
ROW_BLOCKS = [(n, 200) for n in (257, 288, 289, 320, 321)]      # wave 0 with one row tile / both / wave 1 with one row tile
GRID = [(a, b) for a in (200, 300, 600) for b in (200, 300, 600)]  # 1, 2, 3 chunks x 1, 2, 3 row blocks (3: the odd last step)
CARRY = [(1000, 777), (600, 2000)]                              # several chunks, an odd row-block count
SIZES = _both_orders(TILE_EDGES + QUERY_TILES + ROW_BLOCKS + GRID + CARRY + [(2000, 2000)])


def _batched(f1, f2, cfg=None):
    """the pair (0, 1) through match_pairs without the robust stage: (counts, matches, timings)"""
    from opensfm_amd._lib import MatchTimings

    store = matching.DescriptorStore([f1, f2], [np.zeros((len(f1), 2)), np.zeros((len(f2), 2))])
    tm = MatchTimings()
    counts, m = matching.match_pairs(store, np.array([[0, 1]], np.int32), cfg or {}, robust=False, timings=tm)
    counts, m = counts.copy(), m.copy()
    store.close()
    return counts, m, tm


@pytest.mark.parametrize("n1,n2", SIZES)
def test_partial_steps_equal_oracle(oracle_lib, gpu_ctx, n1, n2):
    f1, f2 = _pair(n1, n2, 1000 * n1 + n2)
    cfg = {"lowes_ratio": 0.8}
    want = _tuples(oracle_lib.match_brute_force_symmetric(f1, f2))
    assert matching.match_brute_force_symmetric(f1, f2, cfg) == want
    assert matching.match_brute_force(f1, f2, cfg) == _tuples(oracle_lib.match_brute_force(f1, f2))
    counts, m, _ = _batched(f1, f2)
    offsets = np.array([0, n1, n1 + n2])
    wantp = oracle_lib.match_pairs(np.concatenate([f1, f2]), np.zeros((n1 + n2, 2)), offsets, np.array([[0, 1]], np.int32), stage=0)
    assert int(counts[0]) == len(wantp[0])
    assert _tuples(m) == _tuples(wantp[0])
    if min(n1, n2) >= 16:
        assert len(want) >= min(n1, n2) // 4  # the planted copies are found: pass B and the emission ran


def test_ragged_store_all_pairs_with_an_unrelated_image(oracle_lib, gpu_ctx):
    """counts 1 (the n < 2 early return), 2, 33, 225, 257, 600; the image of 225 shares nothing with the others, so its pairs end
    empty through the tail skip"""
    rng = np.random.default_rng(5)
    ns = [1, 2, 33, 225, 257, 600]
    base = synthetic._hahog_like(rng, 600).astype(np.float32)
    imgs = []
    for i, n in enumerate(ns):
        if n == 225:
            imgs.append(synthetic._hahog_like(np.random.default_rng(99), n).astype(np.float32))
        else:
            imgs.append(np.clip(base[rng.permutation(600)[:n]] + np.rint(rng.normal(0, 3, (n, 128))), 0, 255).astype(np.float32))
    desc = np.concatenate(imgs)
    offsets = np.concatenate([[0], np.cumsum(ns)])
    pts = np.zeros((len(desc), 2))
    pairs = synthetic.all_pairs(len(ns))
    store = matching.DescriptorStore.from_packed(desc, pts, offsets)
    counts, m = matching.match_pairs(store, pairs, robust=False)
    want = oracle_lib.match_pairs(desc, pts, offsets, pairs, stage=0)
    got = matching.split_matches(counts, m)
    assert [len(g) for g in got] == [len(w) for w in want]
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    k = ns.index(225)
    empty = [i for i, (a, b) in enumerate(pairs) if k in (a, b) and min(ns[a], ns[b]) >= 33]
    assert len(empty) >= 3
    for i in empty:
        assert counts[i] == 0 and len(want[i]) == 0
    assert sum(len(w) for w in want) > 150
    store.close()


def test_hits_in_pass_a_but_nothing_mutual(oracle_lib, gpu_ctx):
    """two identical rows of image 1 equal row j of image 2 and a third row of image 1 is a noisy copy of it: every row of image 1
    finds j, but j's two nearest neighbours in image 1 are at the same distance, so nothing is mutual.  In the order (f2, f1) the
    kernel's first pass (queries: the pair's second image) has hits and the second pass leaves none; in the order (f1, f2) the first
    pass already ends empty."""
    rng = np.random.default_rng(8)
    f1 = rng.integers(60, 196, (300, 128)).astype(np.float32)
    f2 = rng.integers(0, 30, (260, 128)).astype(np.float32)  # far background
    j = 77
    f2[j] = f1[10]
    f1[141] = f1[10]
    f1[290] = np.clip(f1[10] + rng.integers(-2, 3, 128), 0, 255)
    cfg = {"lowes_ratio": 0.8}
    for a, b in ((f1, f2), (f2, f1)):
        one = oracle_lib.match_brute_force(f1, f2)
        sym = oracle_lib.match_brute_force_symmetric(a, b)
        assert len(one) > 0 and len(sym) == 0
        assert matching.match_brute_force(f1, f2, cfg) == _tuples(one)
        assert matching.match_brute_force_symmetric(a, b, cfg) == []
        counts, m, _ = _batched(a, b)
        assert counts[0] == 0 and len(m) == 0


def _root_features(desc_u8):
    d = desc_u8.astype(np.float32)
    d /= np.maximum(d.sum(1, keepdims=True), 1e-7)
    return np.sqrt(d).astype(np.float32)


@pytest.mark.parametrize("n1,n2", _both_orders(TILE_EDGES + QUERY_TILES) + [(600, 600)])
def test_partial_steps_float_store(oracle_lib, gpu_ctx, n1, n2):
    """the float store (FQ instantiation of the kernel) on root descriptors, against the oracle's float matcher"""
    rng = np.random.default_rng(n1 * 7 + n2)
    base = rng.integers(0, 120, (max(n1, n2), 128))
    f1 = _root_features(np.clip(base[:n1] + rng.integers(-3, 4, (n1, 128)), 0, 255))
    f2 = _root_features(np.clip(base[:n2] + rng.integers(-3, 4, (n2, 128)), 0, 255))
    cfg = {"lowes_ratio": 0.8}
    assert matching.match_brute_force(f1, f2, cfg) == _tuples(oracle_lib.match_brute_force(f1, f2, 0.8))
    sym = matching.match_brute_force_symmetric(f1, f2, cfg)
    assert sorted(sym) == sorted(_tuples(oracle_lib.match_brute_force_symmetric(f1, f2, 0.8)))
    if min(n1, n2) >= 31:
        assert len(sym) >= min(n1, n2) // 2


def test_collision_flag_survives_an_empty_pair(oracle_lib, gpu_ctx):
    """descriptors at 0 / 255 (every d^2 > 2^22) with a ratio nothing passes: the pair skips its tail, and is still flagged and re-run
    on the exact kernel"""
    rng = np.random.default_rng(12)
    f1 = rng.integers(0, 9, (200, 128)).astype(np.float32)
    f2 = (255 - rng.integers(0, 9, (200, 128))).astype(np.float32)
    counts, m, tm = _batched(f1, f2, {"lowes_ratio": 0.5})
    want = oracle_lib.match_brute_force_symmetric(f1, f2, 0.5)
    assert tm.pairs_exact_path == 1
    assert len(want) == 0 and counts[0] == 0 and len(m) == 0
