"""Match graphs that stress ``opensfm_amd/csrc/tracks.hip`` and the independent truth they are compared with.

``reference_from_edges`` is the reference's own procedure (opensfm/tracking.py:82-98 and ``_good_track``, on the union-find of
opensfm/unionfind.py:67-103 as transcribed in ``tests/test_oracle_tracks.py``) run over ``(image, feature)`` tuples in edge order.  It
never calls the oracle or the library and knows nothing of the GPU formulation (no rank, no hooking, no sort).

``CASES`` names seeded generators of ``(edge_a, edge_b, node_offsets, min_length)``.  What the kernels can get wrong decides the sizes:
one component of 2^18 / 20 000 nodes makes thousands of hooks race on one tree (long parent chains before compression, roots that lose a
compare-and-swap and climb, redundant edges inside a merged component); the ragged scenes put empty images in front, between and behind
(``image_of`` sees ``off[k] == off[k + 1]``), many components (a wrong root renumbers the later tracks) and repeated images; the pair
cases put segment heads on both sides of the 256-thread block boundaries ``head_kernel`` / ``dup_kernel`` look across.
"""
import functools

import numpy as np

from test_oracle_tracks import _UnionFind


def reference_from_edges(ea, eb, off, min_length):
    """-> (tracks, stats): the good tracks as lists of ``(image, feature)`` in the reference's order, and how many components there were
    (``components``), how many fell for their length (``too_short``) and how many for a repeated image (``repeated_image``)"""
    off = np.asarray(off, np.int64)
    nodes = np.stack([np.asarray(ea, np.int64), np.asarray(eb, np.int64)], axis=1)
    image = np.searchsorted(off, nodes, side="right") - 1  # the image whose [off[k], off[k + 1]) holds the node; empty images hold none
    feature = nodes - off[image]
    a = list(zip(image[:, 0].tolist(), feature[:, 0].tolist()))
    b = list(zip(image[:, 1].tolist(), feature[:, 1].tolist()))
    uf = _UnionFind()
    for x, y in zip(a, b):
        uf.union(x, y)
    sets = {}
    for i in uf:
        p = uf[i]
        if p in sets:
            sets[p].append(i)
        else:
            sets[p] = [i]
    tracks, too_short, repeated = [], 0, 0
    for t in sets.values():
        if len(t) < min_length:
            too_short += 1
            continue
        images = [f[0] for f in t]
        if len(images) != len(set(images)):
            repeated += 1
            continue
        tracks.append(t)
    return tracks, {"components": len(sets), "too_short": too_short, "repeated_image": repeated}


# ---------------------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------------------
def _orient(rng, a, b):
    """every edge handed over in a random direction"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    flip = rng.random(len(a)) < 0.5
    return np.where(flip, b, a).astype(np.int32), np.where(flip, a, b).astype(np.int32)


def _one_feature_images(n):
    return np.arange(n + 1, dtype=np.int64)


def path(n, order, seed=0):
    """one path over n images of one feature each; the edges ascending ("fwd"), descending ("rev") or shuffled"""
    rng = np.random.default_rng(seed)
    lo = np.arange(n - 1)
    if order == "rev":
        lo = lo[::-1]
    elif order == "shuffled":
        lo = rng.permutation(lo)
    ea, eb = _orient(rng, lo, lo + 1)
    return ea, eb, _one_feature_images(n), 2


def star(n, centre, seed=1):
    """every other node linked to `centre`, the leaves in random order"""
    rng = np.random.default_rng(seed)
    leaves = rng.permutation(np.delete(np.arange(n), centre))
    ea, eb = _orient(rng, leaves, np.full(n - 1, centre))
    return ea, eb, _one_feature_images(n), 2


def binary_tree(n, shuffled, seed=2):
    """node c linked to (c - 1) // 2"""
    rng = np.random.default_rng(seed)
    c = np.arange(1, n)
    if shuffled:
        c = rng.permutation(c)
    ea, eb = _orient(rng, c, (c - 1) // 2)
    return ea, eb, _one_feature_images(n), 2


def two_halves(n, join_first, seed=3):
    """two paths of n / 2 nodes, their edges shuffled together, and one edge that joins them: the last of the list, or the first"""
    rng = np.random.default_rng(seed)
    h = n // 2
    lo = rng.permutation(np.r_[np.arange(h - 1), h + np.arange(h - 1)])
    a, b = lo, lo + 1
    join = ([h - 1], [h])
    a, b = (np.r_[join[0], a], np.r_[join[1], b]) if join_first else (np.r_[a, join[0]], np.r_[b, join[1]])
    ea, eb = _orient(rng, a, b)
    return ea, eb, _one_feature_images(n), 2


def clique(n, seed=4):
    """all pairs of n one-feature images: one track of length n under heavy redundant hooking"""
    rng = np.random.default_rng(seed)
    a, b = np.triu_indices(n, 1)
    order = rng.permutation(len(a))
    ea, eb = _orient(rng, a[order], b[order])
    return ea, eb, _one_feature_images(n), 2


def pairs_at_block_edges(n, lead_triple=False, seed=5):
    """n // 2 disjoint two-node tracks over n one-feature images, in shuffled order (an odd n leaves its last node in no match): in the
    sorted member list the segment heads sit at the even positions, so that 254|256 and 256|258 straddle the 256-thread block boundary.
    `lead_triple` makes the first track three nodes long instead (it uses the last node), which moves every later head to an odd
    position: 255|257."""
    rng = np.random.default_rng(seed + n)
    first = np.arange(n // 2) * 2
    order = rng.permutation(len(first))
    a, b = _orient(rng, first[order], first[order] + 1)
    if lead_triple:
        assert n % 2 == 1
        a, b = np.r_[a[:1], a[0], a[1:]].astype(np.int32), np.r_[b[:1], n - 1, b[1:]].astype(np.int32)
    return a, b, _one_feature_images(n), 2


@functools.lru_cache(maxsize=None)
def _ragged_scene(seed):
    rng = np.random.default_rng(seed)
    n_images = 64
    counts = rng.integers(1, 900, n_images)
    empty = rng.random(n_images) < 0.2
    empty[[0, n_images // 2, n_images - 1]] = True
    counts[empty] = 0
    off = np.r_[0, np.cumsum(counts)].astype(np.int64)
    fresh = [list(rng.permutation(int(c))) for c in counts]  # every image hands each of its features out once, in random order
    ea, eb = [], []
    for _ in range(4000):
        open_images = np.flatnonzero([len(f) > 0 for f in fresh])
        k = int(rng.integers(2, 9))
        if len(open_images) < k:
            break
        nodes = [off[im] + fresh[im].pop() for im in rng.choice(open_images, k, replace=False)]
        for i in range(k):
            for j in range(i + 1, k):
                if rng.random() < 0.7:
                    ea.append(nodes[i])
                    eb.append(nodes[j])
    n_extra = int(0.03 * len(ea))  # links between random nodes: they merge tracks, and most merged tracks see an image twice
    ea = np.r_[ea, rng.integers(0, off[-1], n_extra)]
    eb = np.r_[eb, rng.integers(0, off[-1], n_extra)]
    order = rng.permutation(len(ea))
    ea, eb = _orient(rng, ea[order], eb[order])
    for x in (ea, eb, off):
        x.setflags(write=False)
    return ea, eb, off


def ragged_scene(seed, min_length):
    """64 images with 0 .. 899 features (about 20 % empty, the first, the middle and the last one always), 4000 tracks over 2 .. 8
    distinct non-empty images on fresh features, each pair inside a track linked with probability 0.7, 3 % extra links between random
    nodes; shuffled and randomly oriented"""
    return _ragged_scene(seed) + (min_length,)


def duplicates(seed=0):
    """the first 5000 edges of a ragged scene, three times over"""
    ea, eb, off = _ragged_scene(seed)
    return np.tile(ea[:5000], 3), np.tile(eb[:5000], 3), off, 2


def self_loops(min_length, seed=1):
    """a ragged scene plus 2 % edges (a, a) on random nodes, shuffled in"""
    ea, eb, off = _ragged_scene(seed)
    rng = np.random.default_rng(100 + seed)
    loops = rng.integers(0, off[-1], int(0.02 * len(ea))).astype(np.int32)
    order = rng.permutation(len(ea) + len(loops))
    return np.r_[ea, loops][order], np.r_[eb, loops][order], off, min_length


_GAPS = np.array([0, 0, 4, 4, 9, 9], np.int64)  # images 0, 2 and 4 are empty: in front, between and behind


def tiny(edges, off, min_length):
    return np.array(edges[0], np.int32), np.array(edges[1], np.int32), np.asarray(off, np.int64), min_length


CASES = [
    ("path_fwd", functools.partial(path, 20000, "fwd")),
    ("path_rev", functools.partial(path, 20000, "rev")),
    ("path_shuffled", functools.partial(path, 2 ** 18, "shuffled")),
    ("star_first", functools.partial(star, 20000, 0)),
    ("star_last", functools.partial(star, 20000, 19999)),
    ("binary_tree", functools.partial(binary_tree, 20000, False)),
    ("binary_tree_shuffled", functools.partial(binary_tree, 20000, True)),
    ("two_halves", functools.partial(two_halves, 20000, False)),
    ("two_halves_join_first", functools.partial(two_halves, 20000, True)),
    ("clique", functools.partial(clique, 600)),
    ("pairs_at_block_edges_512", functools.partial(pairs_at_block_edges, 512)),
    ("pairs_at_block_edges_513", functools.partial(pairs_at_block_edges, 513)),
    ("pairs_at_block_edges_511", functools.partial(pairs_at_block_edges, 511)),
    ("pairs_at_block_edges_513_lead_triple", functools.partial(pairs_at_block_edges, 513, True)),
    ("ragged_scene_0_min2", functools.partial(ragged_scene, 0, 2)),
    ("ragged_scene_0_min4", functools.partial(ragged_scene, 0, 4)),
    ("ragged_scene_1_min2", functools.partial(ragged_scene, 1, 2)),
    ("ragged_scene_1_min4", functools.partial(ragged_scene, 1, 4)),
    ("duplicates", duplicates),
    ("self_loops_min1", functools.partial(self_loops, 1)),
    ("self_loops_min2", functools.partial(self_loops, 2)),
    ("tiny_one_image_min1", functools.partial(tiny, ([0, 3, 3], [0, 3, 3]), [0, 5], 1)),
    ("tiny_one_image_min2", functools.partial(tiny, ([0, 3, 3], [0, 3, 3]), [0, 5], 2)),
    ("tiny_gaps_min1", functools.partial(tiny, ([1, 5, 2], [1, 5, 6]), _GAPS, 1)),
    ("tiny_gaps_min2", functools.partial(tiny, ([1, 5, 2], [1, 5, 6]), _GAPS, 2)),
    ("tiny_gaps_reversed", functools.partial(tiny, ([0, 8], [8, 0]), _GAPS, 2)),
    ("tiny_gaps_repeated", functools.partial(tiny, ([3, 3, 3], [4, 4, 4]), _GAPS, 2)),
]
CASE_NAMES = [name for name, _ in CASES]
ONE_TRACK_CASES = [n for n in CASE_NAMES if n.split("_")[0] in ("path", "star", "binary", "two", "clique")]
RAGGED_CASES = [n for n in CASE_NAMES if n.startswith("ragged_scene")]


@functools.lru_cache(maxsize=None)
def case(name):
    """(edge_a, edge_b, node_offsets, min_length) of a named case, built once per session and read-only"""
    ea, eb, off, min_length = dict(CASES)[name]()
    ea, eb, off = np.ascontiguousarray(ea, np.int32), np.ascontiguousarray(eb, np.int32), np.ascontiguousarray(off, np.int64)
    for x in (ea, eb, off):
        x.setflags(write=False)
    return ea, eb, off, min_length


@functools.lru_cache(maxsize=None)
def reference(name):
    """(tracks, stats) of a named case, computed once per session"""
    return reference_from_edges(*case(name))


def reference_arrays(name):
    """the reference of a named case as (n_tracks, obs_track, obs_image, obs_feature)"""
    tracks, _ = reference(name)
    flat = np.array([(k, im, f) for k, t in enumerate(tracks) for im, f in t], np.int32).reshape(-1, 3)
    return len(tracks), flat[:, 0], flat[:, 1], flat[:, 2]
