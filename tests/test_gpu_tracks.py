"""GPU parity: tracks creation (connected components + _good_track) == CPU oracle, observation by
observation, including the reference's track numbering and member order."""
import numpy as np
import pytest

from test_oracle_tracks import random_match_graph, reference_tracks, to_edges

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_images,n_feat,n_pairs,per_pair,min_length,seed",
                         [(6, 40, 10, 15, 2, 0), (12, 100, 40, 30, 2, 1), (20, 60, 120, 25, 3, 2), (40, 500, 400, 200, 2, 3),
                          (100, 2000, 1500, 600, 2, 4)])
def test_tracks_equal_oracle(oracle_lib, gpu_ctx, n_images, n_feat, n_pairs, per_pair, min_length, seed):
    from opensfm_amd import tracking

    rng = np.random.default_rng(seed)
    matches = random_match_graph(rng, n_images, n_feat, n_pairs, per_pair)
    ea, eb, off = to_edges(matches, n_images, n_feat)
    nt_o, ot_o, oi_o, of_o = oracle_lib.tracks(ea, eb, off, min_length)
    nt_g, ot_g, oi_g, of_g = tracking.create_tracks_arrays(ea, eb, off, min_length)
    assert nt_g == nt_o
    assert np.array_equal(ot_g, ot_o) and np.array_equal(oi_g, oi_o) and np.array_equal(of_g, of_o)


def test_create_tracks_manager_signature(oracle_lib, gpu_ctx):
    """Same call as tracking.create_tracks_manager (tracking.py:68-78) on a dict of matches."""
    from opensfm_amd import tracking

    rng = np.random.default_rng(9)
    m = random_match_graph(rng, 8, 50, 20, 20)
    names = [f"im{i:02d}.jpg" for i in range(8)]
    matches = {(names[a], names[b]): v for (a, b), v in m.items()}
    features = {n: np.zeros((50, 3)) for n in names}
    tm = tracking.create_tracks_manager(features, {}, {}, {}, matches, 2, {})
    ref = reference_tracks(matches, 2)
    assert tm.num_tracks() == len(ref)
    for k, t in enumerate(ref):
        assert tm.get_track_observations(str(k)) == {im: f for im, f in t}


def test_tracks_edge_cases(gpu_ctx):
    from opensfm_amd import tracking

    off = np.array([0, 5, 10, 15], np.int64)
    nt, ot, oi, of = tracking.create_tracks_arrays(np.zeros(0, np.int32), np.zeros(0, np.int32), off, 2)
    assert nt == 0 and len(ot) == 0
    nt, ot, oi, of = tracking.create_tracks_arrays(np.array([1, 7]), np.array([7, 13]), off, 2)
    assert nt == 1 and list(oi) == [0, 1, 2] and list(of) == [1, 2, 3]
    nt, *_ = tracking.create_tracks_arrays(np.array([1, 7, 4]), np.array([7, 13, 13]), off, 2)
    assert nt == 0


@pytest.mark.gpu
def test_gpu_reproduces_the_reference_tracks():
    """The committed output of the reference's own create_tracks_manager (tests/golden/tracks_golden.json)."""
    import test_oracle_tracks as t

    from opensfm_amd import tracking

    t.check_against_golden(tracking.create_tracks_manager)


# ---------------------------------------------------------------------------------------------------------------------------------
# adversarial match graphs (tests/tracks_cases.py), the hand-off from the matcher's arrays, ragged feature stores, argument errors
# ---------------------------------------------------------------------------------------------------------------------------------
import tracks_cases as tc  # noqa: E402
from test_oracle_tracks import check_equal  # noqa: E402


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_adversarial_graphs_equal_the_reference(gpu_ctx, name):
    """Components of up to 2^18 nodes hooked by racing threads, empty images, self-matches, duplicates: the four outputs equal the
    transcription of the reference (tests/tracks_cases.py::reference_from_edges; its premises are pinned in
    tests/test_tracks_cases_host.py), and a second call returns the same bytes."""
    from opensfm_amd import tracking

    ea, eb, off, min_length = tc.case(name)
    nt_r, ot_r, oi_r, of_r = tc.reference_arrays(name)
    first = tracking.create_tracks_arrays(ea, eb, off, min_length, gpu_ctx)
    second = tracking.create_tracks_arrays(ea, eb, off, min_length, gpu_ctx)
    nt, ot, oi, of = first
    assert nt == nt_r and len(ot) == len(ot_r)
    assert np.array_equal(ot, ot_r)
    assert np.array_equal(oi, oi_r)
    assert np.array_equal(of, of_r)
    assert second[0] == nt
    for x, y in zip(first[1:], second[1:]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def _ragged_match_graph(seed=21, n_images=12):
    """(pairs, counts, matches, offsets) in the layout matching.match_pairs returns: int32 pair list, int32 count per pair, the (i, j)
    feature indices of all pairs concatenated.  Images hold 0 .. 59 features (the first two are empty), a third of the pairs have no
    match, and a pair of an empty image never has one."""
    rng = np.random.default_rng(seed)
    n_feat = rng.integers(1, 60, n_images)
    n_feat[[0, 1]] = 0
    off = np.r_[0, np.cumsum(n_feat)].astype(np.int64)
    a, b = np.triu_indices(n_images, 1)
    order = rng.permutation(len(a))[:40]
    pairs = np.stack([a[order], b[order]], axis=1).astype(np.int32)
    counts, blocks = [], []
    for k, (i, j) in enumerate(pairs):
        cap = min(n_feat[i], n_feat[j])
        c = 0 if (k % 3 == 1 or cap == 0) else int(rng.integers(1, cap + 1))
        # mostly f -> f links, a fifth of them to a random feature: merged and repeated-image components
        fi = rng.choice(n_feat[i], c, replace=False) if c else np.zeros(0, np.int64)
        fj = np.where(rng.random(c) < 0.2, rng.integers(0, max(n_feat[j], 1), c), np.minimum(fi, max(n_feat[j] - 1, 0)))
        counts.append(c)
        blocks.append(np.stack([fi, fj], axis=1).astype(np.int32).reshape(-1, 2))
    return pairs, np.array(counts, np.int32), np.concatenate(blocks), off


def test_match_graph_hand_off(gpu_ctx):
    """tracking.edges_from_match_graph: the matcher's (pairs, counts, matches) arrays become the node ids create_tracks_manager builds pair
    by pair, and the tracks over them are those of the reference run on the same matches as a dict."""
    from opensfm_amd import tracking
    from opensfm_amd._lib import OsfmError

    pairs, counts, matches, off = _ragged_match_graph()
    assert (counts == 0).sum() >= 10 and (counts > 0).sum() >= 10 and len(set(counts.tolist())) > 5 and counts.sum() == len(matches)
    assert len(set(np.diff(off).tolist())) > 5 and (np.diff(off) == 0).sum() == 2
    ea, eb = tracking.edges_from_match_graph(pairs, counts, matches, off)
    assert ea.dtype == np.int32 and eb.dtype == np.int32
    # the per-pair concatenation of create_tracks_manager (tracking.py: off[index[im1]] + m[:, 0] for every pair, in order)
    split = np.split(matches.astype(np.int64), np.cumsum(counts)[:-1])
    want_a = np.concatenate([off[i] + m[:, 0] for (i, j), m in zip(pairs, split)])
    want_b = np.concatenate([off[j] + m[:, 1] for (i, j), m in zip(pairs, split)])
    assert np.array_equal(ea, want_a) and np.array_equal(eb, want_b)
    as_dict = {(int(i), int(j)): [(int(x), int(y)) for x, y in m] for (i, j), m in zip(pairs, split)}
    assert len(as_dict) == len(pairs)
    ref = reference_tracks(as_dict, 2)
    assert len(ref) >= 20 and max(len(t) for t in ref) >= 4
    check_equal(ref, tracking.create_tracks_arrays(ea, eb, off, 2, gpu_ctx))
    forged = off.copy()
    forged[-1] = 2 ** 31
    with pytest.raises(OsfmError):
        tracking.edges_from_match_graph(pairs, counts, matches, forged)
    forged[-1] = 2 ** 31 - 1  # the last size that fits
    ea2, eb2 = tracking.edges_from_match_graph(pairs, counts, matches, forged)
    assert np.array_equal(ea2, ea) and np.array_equal(eb2, eb)


def test_create_tracks_manager_on_ragged_features(gpu_ctx):
    """Row counts that differ between images, an image of `matches` without a `features` entry (the reference skips its observations,
    tracking.py:105-107, and keeps the track ids) and an image with features but no match."""
    from opensfm_amd import tracking

    pairs, counts, m, off = _ragged_match_graph(seed=22)
    names = ["im%02d.jpg" % i for i in range(len(off) - 1)]
    split = np.split(m, np.cumsum(counts)[:-1])
    matches = {(names[i], names[j]): [(int(x), int(y)) for x, y in mm] for (i, j), mm in zip(pairs, split)}
    used = [n for n in names if any(n in k and len(v) for k, v in matches.items())]
    absent = used[3]
    features = {n: np.zeros((int(off[i + 1] - off[i]) + i, 3)) for i, n in enumerate(names) if n != absent}  # more rows than the matches use
    features["unmatched.jpg"] = np.zeros((17, 3))
    assert len({len(f) for f in features.values()}) > 5
    ref = reference_tracks(matches, 2)
    assert any(im == absent for tr in ref for im, _ in tr) and len(ref) >= 20
    tm = tracking.create_tracks_manager(features, {}, {}, {}, matches, 2, {}, ctx=gpu_ctx)
    assert tm.num_tracks() == len(ref) and tm.get_track_ids() == [str(k) for k in range(len(ref))]
    by_shot = {}
    for k, tr in enumerate(ref):
        kept = {im: f for im, f in tr if im in features}
        assert absent not in kept and len(kept) >= 1
        assert tm.get_track_observations(str(k)) == kept
        assert list(tm.get_track_observations(str(k)).items()) == list(kept.items())  # members in the reference's order
        for im, f in kept.items():
            by_shot.setdefault(im, {})[str(k)] = f
    assert tm.num_observations() == sum(len(v) for v in by_shot.values())
    assert set(tm.get_shot_ids()) == set(by_shot) and absent not in tm.get_shot_ids() and "unmatched.jpg" not in tm.get_shot_ids()
    for im, obs in by_shot.items():
        assert tm.get_shot_observations(im) == obs
    assert tm.get_shot_observations(absent) == {}


def test_documented_errors(gpu_ctx):
    """osfm_tracks_create's argument checks: a node id outside [0, N) is OSFM_E_INVALID and osfm_last_error names the match; null
    pointers are refused; the Python layer refuses ids that the int32 cast would wrap; the context still works afterwards."""
    import ctypes as C

    from opensfm_amd import _lib, tracking

    lib = _lib.load()
    E_INVALID = -1  # OSFM_E_INVALID, include/osfm_mi355.h
    off = np.array([0, 5, 10, 15], np.int64)
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def create(ea, eb, off_ptr=off.ctypes.data_as(i64), out=True):
        ea, eb = np.array(ea, np.int32), np.array(eb, np.int32)
        h = C.c_void_p()
        status = lib.osfm_tracks_create(gpu_ctx.handle, ea.ctypes.data_as(i32), eb.ctypes.data_as(i32), len(ea), off_ptr, 3, 2,
                                        C.byref(h) if out else None)
        assert h.value is None or status == 0
        if h.value is not None:
            lib.osfm_tracks_destroy(h)
        return status, (lib.osfm_last_error() or b"").decode()

    status, msg = create([1, 7, 3], [7, 13, 15])  # 15 == N
    assert status == E_INVALID and "match 2" in msg and "15" in msg
    status, msg = create([1, -4], [7, 13])
    assert status == E_INVALID and "match 1" in msg and "-4" in msg
    status, msg = create([1, 7], [-1, 13])
    assert status == E_INVALID and "match 0" in msg and "-1" in msg
    assert create([1], [7], out=False)[0] == E_INVALID
    assert create([1], [7], off_ptr=None)[0] == E_INVALID
    h = C.c_void_p()
    assert lib.osfm_tracks_create(gpu_ctx.handle, None, None, 1, off.ctypes.data_as(i64), 3, 2, C.byref(h)) == E_INVALID and h.value is None
    assert lib.osfm_tracks_create(None, None, None, 0, off.ctypes.data_as(i64), 3, 2, C.byref(h)) == E_INVALID
    # through Python: ids the int32 cast would wrap into valid ones (2^32 + 1 -> 1), and the plain out-of-range ones
    for bad in (2 ** 32 + 1, 2 ** 31, -1, -(2 ** 32) + 1):
        with pytest.raises(_lib.OsfmError):
            tracking.create_tracks_arrays(np.array([1, bad], np.int64), np.array([7, 13], np.int64), off, 2, gpu_ctx)
        with pytest.raises(_lib.OsfmError):
            tracking.create_tracks_arrays(np.array([1, 7], np.int64), np.array([7, bad], np.int64), off, 2, gpu_ctx)
    with pytest.raises(_lib.OsfmError, match="match 1"):
        tracking.create_tracks_arrays(np.array([1, 15]), np.array([7, 13]), off, 2, gpu_ctx)
    forged = off.copy()
    forged[-1] = 2 ** 31
    with pytest.raises(_lib.OsfmError):
        tracking.create_tracks_arrays(np.array([1]), np.array([7]), forged, 2, gpu_ctx)
    nt, ot, oi, of = tracking.create_tracks_arrays(np.array([1, 7]), np.array([7, 13]), off, 2, gpu_ctx)
    assert nt == 1 and list(ot) == [0, 0, 0] and list(oi) == [0, 1, 2] and list(of) == [1, 2, 3]
