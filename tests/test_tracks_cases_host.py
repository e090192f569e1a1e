"""The cases of ``tests/tracks_cases.py`` on the CPU: the oracle (oracle/tracks_oracle.c) equals the transcription of the reference on
every one, and the cases are what the GPU test takes them for.  The premises below are conditions on the transcription alone; they keep
a generator that drifts from making ``test_gpu_tracks.py::test_adversarial_graphs_equal_the_reference`` vacuous."""
import numpy as np
import pytest

import tracks_cases as tc
from test_oracle_tracks import check_equal


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_oracle_equals_the_transcription(oracle_lib, name):
    ea, eb, off, min_length = tc.case(name)
    tracks, _ = tc.reference(name)
    check_equal(tracks, oracle_lib.tracks(ea, eb, off, min_length))


def test_every_case_is_listed_once_and_well_formed():
    assert len(set(tc.CASE_NAMES)) == len(tc.CASE_NAMES)
    for name in tc.CASE_NAMES:
        ea, eb, off, min_length = tc.case(name)
        assert ea.dtype == np.int32 and eb.dtype == np.int32 and off.dtype == np.int64 and len(ea) == len(eb) > 0
        assert off[0] == 0 and (np.diff(off) >= 0).all() and min_length >= 1
        assert ea.min() >= 0 and eb.min() >= 0 and max(ea.max(), eb.max()) < off[-1]


def test_sizes_are_those_the_races_need():
    sizes = {name: int(tc.case(name)[2][-1]) for name in tc.ONE_TRACK_CASES}
    assert sizes.pop("path_shuffled") == 2 ** 18 and sizes.pop("clique") == 600
    assert len(tc.case("clique")[0]) == 179700
    assert len(sizes) == 8 and set(sizes.values()) == {20000}


@pytest.mark.parametrize("name", tc.ONE_TRACK_CASES)
def test_one_component_cases_are_one_track_of_every_node(name):
    ea, eb, off, _ = tc.case(name)
    tracks, stats = tc.reference(name)
    assert stats == {"components": 1, "too_short": 0, "repeated_image": 0}
    assert len(tracks) == 1 and sorted(tracks[0]) == [(i, 0) for i in range(int(off[-1]))]
    # the listing starts at the first node of the first edge, whichever node the union-find made the root
    assert tracks[0][0] == (int(ea[0]), 0) and tracks[0][1] == (int(eb[0]), 0)


@pytest.mark.parametrize("n", [512, 513, 511])
def test_pair_cases_put_heads_on_both_sides_of_the_block_boundary(n):
    tracks, stats = tc.reference("pairs_at_block_edges_%d" % n)
    assert [len(t) for t in tracks] == [2] * (n // 2) and stats["components"] == n // 2
    if n == 513:
        tracks, _ = tc.reference("pairs_at_block_edges_513_lead_triple")
        assert [len(t) for t in tracks] == [3] + [2] * 255  # heads at 0, 3, 5, ..., 255, 257, ...


@pytest.mark.parametrize("name", tc.RAGGED_CASES)
def test_ragged_scene_premises(name):
    ea, eb, off, min_length = tc.case(name)
    tracks, stats = tc.reference(name)
    counts = np.diff(off)
    assert len(counts) == 64 and (counts == 0).sum() >= 10 and counts[0] == 0 and counts[32] == 0 and counts[63] == 0
    assert counts.max() < 900 and len(set(counts.tolist())) > 40  # ragged
    assert len(tracks) >= 1000
    assert stats["repeated_image"] >= 0.02 * stats["components"]
    if min_length == 4:
        assert stats["too_short"] >= 0.20 * stats["components"]
    assert max(len(t) for t in tracks) > 8
    # both orientations and every empty image's boundary value occur among the nodes' neighbours: feature 0 of an image that follows
    # an empty one is where a wrong comparison in the image search shows
    after_empty = off[1:-1][(counts[:-1] == 0) & (counts[1:] > 0)]
    assert np.isin(after_empty, np.r_[ea, eb]).any()
    assert (ea < eb).any() and (ea > eb).any()


def test_self_loop_premises():
    t1, s1 = tc.reference("self_loops_min1")
    t2, s2 = tc.reference("self_loops_min2")
    assert (tc.case("self_loops_min1")[0] == tc.case("self_loops_min1")[1]).sum() >= 100
    assert sum(len(t) == 1 for t in t1) >= 1
    assert all(len(t) >= 2 for t in t2) and s2["too_short"] >= 1
    assert [t for t in t1 if len(t) >= 2] == t2 and s1["components"] == s2["components"]


def test_duplicates_give_the_tracks_of_the_deduplicated_list():
    ea, eb, off, min_length = tc.case("duplicates")
    assert len(ea) == 15000 and np.array_equal(ea[:5000], ea[5000:10000]) and np.array_equal(eb[:5000], eb[10000:])
    once, _ = tc.reference_from_edges(ea[:5000], eb[:5000], off, min_length)
    assert len(once) > 100 and once == tc.reference("duplicates")[0]


def test_tiny_cases_by_hand():
    assert tc.reference("tiny_one_image_min1")[0] == [[(0, 0)], [(0, 3)]]
    assert tc.reference("tiny_one_image_min2")[0] == []
    # off = [0, 0, 4, 4, 9, 9]: nodes 0..3 are image 1, nodes 4..8 image 3
    assert tc.reference("tiny_gaps_min1")[0] == [[(1, 1)], [(3, 1)], [(1, 2), (3, 2)]]
    assert tc.reference("tiny_gaps_min2")[0] == [[(1, 2), (3, 2)]]
    assert tc.reference("tiny_gaps_reversed")[0] == [[(1, 0), (3, 4)]]
    assert tc.reference("tiny_gaps_repeated")[0] == [[(1, 3), (3, 0)]]
