"""GPU parity of the fused matcher's resident grid: min(n_pairs, 2 x CUs) workgroups that draw their pairs by ticket and loop over
them, with the next pair's header fetched under the current pair.  What can go wrong there is state that survives a pair (LDS result
arrays that are no longer cleared per pair, hit words, the flag word, the header slot), tickets that survive a launch, and the ends of
the eight ticket ranges (a workgroup whose own range is used up goes on with the next one).  The store is ~48 tiny ragged images (feature counts around every tile and chunk edge, some with fewer than
two features, which take the early path that must still draw the next ticket), cut out of a street scene so that neighbours truly
match; all its pairs are more than twice the resident grid of a 256-CU part.  Every result is compared with the exact VALU kernels
(OSFM_MATCH_EXACT_KERNEL) on the same pairs, and a subsample with the CPU oracle, for the integer and the float store, symmetric and
both one-way modes.  Which workgroup draws which pair is not deterministic, so the lists are long enough that every workgroup walks
through several pairs, and the same list is also run reversed and shuffled."""
import ctypes as C

import numpy as np
import pytest

from opensfm_amd import _lib, matching, synthetic

pytestmark = pytest.mark.gpu

N_IMAGES = 48
EDGE_COUNTS = [0, 1, 2, 31, 32, 33, 64, 65, 255, 256, 257]
LARGE_COUNTS = [300, 333, 365, 400]
MODES = {"symmetric": {}, "one-way": {"symmetric_matching": False}, "one-way-flann": {"symmetric_matching": False, "matcher_type": "FLANN"}}


def _root_features(desc_u8):
    d = desc_u8.astype(np.float32)
    d /= np.maximum(d.sum(1, keepdims=True), 1e-7)
    return np.sqrt(d).astype(np.float32)


def _match(store, pairs, cfg, exact=False):
    lib = _lib.load()
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    prm = matching.make_params(cfg, robust=False)
    if exact:
        prm.flags |= _lib.MATCH_EXACT_KERNEL
    res = C.c_void_p()
    _lib.check(lib.osfm_match_pairs(store.ctx.handle, store.handle, pairs.ctypes.data_as(C.POINTER(C.c_int32)), len(pairs), C.byref(prm),
                                    C.byref(res), None), "osfm_match_pairs")
    counts, m = matching._fetch_result(lib, res)
    return np.array(counts, np.int32), np.array(m, np.int32).reshape(-1, 2)


class Scene:
    """the ragged store in both descriptor types, and per mode the exact kernels' result for every pair (computed once, never changed)"""

    def __init__(self, ctx):
        sc = synthetic.make_matching_scene(N_IMAGES, 400, seed=77)
        # neighbours in the list of images are neighbours in the scene: edge-sized and large images alternate, so that pairs of
        # every combination (tiny-tiny, tiny-large, large-large) exist among images that see the same points
        self.ns = [(EDGE_COUNTS[(i // 2) % len(EDGE_COUNTS)] if i % 2 else LARGE_COUNTS[(i // 2) % len(LARGE_COUNTS)]) for i in range(N_IMAGES)]
        self.ns[5], self.ns[6] = 256, 257
        rows = np.concatenate([np.arange(sc.offsets[i], sc.offsets[i] + n) for i, n in enumerate(self.ns)]).astype(np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.ns)]).astype(np.int64)
        self.pts = np.ascontiguousarray(sc.pts[rows])
        self.desc = {"int": np.ascontiguousarray(sc.desc[rows]).astype(np.float32), "float": _root_features(sc.desc[rows])}
        self.stores = {k: matching.DescriptorStore.from_packed(d, self.pts, self.offsets, ctx) for k, d in self.desc.items()}
        self.pairs = synthetic.all_pairs(N_IMAGES)
        self.index = {(int(a), int(b)): i for i, (a, b) in enumerate(self.pairs)}
        self.grid = 2 * int(ctx.num_cus)
        self.ref = {}
        for kind, store in self.stores.items():
            for mode, cfg in MODES.items():
                counts, m = _match(store, self.pairs, cfg, exact=True)
                self.ref[kind, mode] = (counts, matching.split_matches(counts, m))

    def expected(self, kind, mode, pairs):
        counts, rows = self.ref[kind, mode]
        idx = [self.index[int(a), int(b)] for a, b in pairs]
        m = [rows[i] for i in idx if len(rows[i])]
        return counts[idx], (np.concatenate(m) if m else np.zeros((0, 2), np.int32))

    def check(self, kind, mode, pairs):
        counts, m = _match(self.stores[kind], pairs, MODES[mode])
        wc, wm = self.expected(kind, mode, pairs)
        assert np.array_equal(counts, wc)
        assert np.array_equal(m, wm)
        return counts

    def cycled(self, n, start=0):
        """n pairs of the store, walking the list of all pairs (and around it when n is larger)"""
        return self.pairs[(start + np.arange(n)) % len(self.pairs)]


@pytest.fixture(scope="module")
def scene(gpu_ctx):
    s = Scene(gpu_ctx)
    yield s
    for store in s.stores.values():
        store.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", ["int", "float"])
def test_all_pairs_equal_exact_kernel(scene, kind, mode):
    """all 1128 pairs: more than two pairs per resident workgroup on a 256-CU part"""
    counts = scene.check(kind, mode, scene.pairs)
    # the premise: pairs with matches (pass B, emission), far more empty ones, and pairs that take the early path
    assert (counts > 0).sum() >= 40 and (counts == 0).sum() >= 500
    assert sum(1 for a, b in scene.pairs if min(scene.ns[a], scene.ns[b]) < 2) >= 100


@pytest.mark.parametrize("kind", ["int", "float"])
def test_subsample_equals_oracle(oracle_lib, scene, kind):
    """every 9th pair and every pair of neighbouring images, fused kernel against the CPU oracle in all three modes"""
    sel = sorted(set(range(0, len(scene.pairs), 9)) | {scene.index[i, i + 1] for i in range(N_IMAGES - 1)} | {scene.index[i, i + 2] for i in range(N_IMAGES - 2)})
    pairs = scene.pairs[sel]
    d, o = scene.desc[kind], scene.offsets
    n_matches = 0
    for mode, cfg in MODES.items():
        counts, m = _match(scene.stores[kind], pairs, cfg)
        got = matching.split_matches(counts, m)
        for (a, b), g in zip(pairs, got):
            f1, f2 = d[o[a]:o[a + 1]], d[o[b]:o[b + 1]]
            if len(f1) < 2 or len(f2) < 2:
                want = np.zeros((0, 2), np.int32)
            elif mode == "symmetric":
                want = oracle_lib.match_brute_force_symmetric(f1, f2, 0.8)
            elif mode == "one-way":
                want = oracle_lib.match_brute_force(f1, f2, 0.8)
            else:
                want = oracle_lib.match_flann(f1, f2, 0.8)
            assert np.array_equal(g, want), (mode, int(a), int(b))
            n_matches += len(want)
    assert n_matches > 300


@pytest.mark.parametrize("kind", ["int", "float"])
def test_list_lengths_around_the_grid(scene, kind):
    """1, grid - 1, grid, grid + 1 and 2 x grid + 3 pairs (grid = 2 x the device's CU count): one workgroup, a grid that is not full,
    exactly one pair per workgroup, one workgroup that has to come back for a second pair, and ranges that do not divide evenly"""
    g = scene.grid
    for k, n in enumerate((1, g - 1, g, g + 1, 2 * g + 3)):
        scene.check(kind, "symmetric", scene.cycled(n, start=97 * k + 46))
    scene.check(kind, "one-way", scene.cycled(2 * g + 3, start=11))
    scene.check(kind, "one-way-flann", scene.cycled(g + 1, start=500))
    for n in range(2, 18):  # fewer pairs than ticket ranges, and the first lists in which a range has two
        scene.check(kind, "symmetric", scene.cycled(n, start=46))


def _sequence(scene, kind):
    """(pair with matches, empty pair, pair with an image of fewer than two features, pair with matches) over and over, each time
    with other pairs, long enough that every resident workgroup walks through several of them"""
    counts = scene.ref[kind, "symmetric"][0]
    small = np.array([min(scene.ns[a], scene.ns[b]) < 2 for a, b in scene.pairs])
    hit, empty, tiny = np.flatnonzero(counts > 0), np.flatnonzero((counts == 0) & ~small), np.flatnonzero(small)
    assert len(hit) >= 40 and len(empty) >= 100 and len(tiny) >= 100
    n = (2 * scene.grid + 3 + 3) // 4
    idx = np.stack([hit[np.arange(n) % len(hit)], empty[np.arange(n) % len(empty)], tiny[np.arange(n) % len(tiny)],
                    hit[(np.arange(n) + 7) % len(hit)]], axis=1).reshape(-1)
    return scene.pairs[idx]


@pytest.mark.parametrize("kind", ["int", "float"])
def test_matches_then_empty_then_tiny_then_matches(scene, kind):
    """the list in its order, reversed and shuffled gives every pair the same result; and so does the same call made twice on one
    context (tickets left behind by a launch would end the second one early)"""
    seq = _sequence(scene, kind)
    first = scene.check(kind, "symmetric", seq)
    again = scene.check(kind, "symmetric", seq)
    assert np.array_equal(first, again)
    scene.check(kind, "symmetric", seq[::-1])
    scene.check(kind, "symmetric", seq[np.random.default_rng(5).permutation(len(seq))])
    scene.check(kind, "one-way", seq)
    scene.check(kind, "one-way-flann", seq[::-1])


@pytest.mark.parametrize("kind", ["int", "float"])
def test_two_chunks_reuse_the_ticket_buffer(scene, kind):
    """9 000 pairs: the batched call splits the list in two chunks, whose launches follow each other on one stream with one ticket
    buffer between them"""
    from opensfm_amd._lib import MatchTimings

    pairs = scene.cycled(9000, start=123)
    tm = MatchTimings()
    counts, m = matching.match_pairs(scene.stores[kind], pairs, {}, robust=False, timings=tm)
    wc, wm = scene.expected(kind, "symmetric", pairs)
    assert tm.match_launches >= 2
    assert np.array_equal(counts, wc)
    assert np.array_equal(np.asarray(m).reshape(-1, 2), wm)
