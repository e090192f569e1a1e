"""osfm_depthmap_prune on the GPU against the numpy restatement of ``DepthmapPruner::Prune`` (tests/prune_cases.py): the four arrays and the
counts byte for byte on the fixtures of tests/test_prune_host.py; the batch against its single calls; a view large enough for the scan of
the block counts to run over several chunks; refusals; ``compat.pydense_full`` called the way opensfm/dense.py calls it."""
import ctypes as C

import numpy as np
import pytest

import prune_cases as cases

pytestmark = pytest.mark.gpu


def run(problems, threshold):
    from opensfm_amd import dense

    return dense.prune_raw(problems, dense.params_from_config({"depthmap_same_depth_threshold": threshold}))


def batch():
    empty_view = {"views": cases.dress([(cases.camera(0, 0), np.eye(3), np.zeros(3), np.zeros((0, 0), np.float32))])}
    problems = [cases.problem(n) for n in ("t001_behind", "one_row", "five_views", "zero_first", "one_pixel", "t001_front")]
    return problems[:2] + [{"views": []}] + problems[2:4] + [empty_view] + problems[4:]


@pytest.mark.parametrize("name", list(cases.FIXTURES) + list(cases.MORE))
def test_pruning_is_byte_equal_to_the_restatement(name):
    """37 x 29 is five pixel blocks of 256, the last one partial; the thresholds are 0.01 and 1.5"""
    want, tally = cases.expected(name)
    got, counts, ms = run([cases.problem(name)], cases.threshold(name))
    assert counts.tolist() == [len(want[3])] and ms > 0.0
    for k, what in enumerate(("points", "normals", "colors", "labels")):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, what
        differ = int((cases.bits(got[k]) != cases.bits(want[k])).sum())
        assert differ == 0, f"{what}: {differ} of {want[k].size} entries differ"
    if name in cases.FIXTURES:  # neither nothing nor everything
        live = cases.live_pixels(cases.problem(name)["views"])
        assert 0.05 * live <= len(want[3]) <= 0.60 * live


def test_the_fixtures_reach_every_branch():
    total = {k: sum(cases.expected(name)[1][k] for name in cases.FIXTURES) for k in cases.TALLY}
    assert all(total[k] > 0 for k in cases.TALLY), total


def test_a_batch_is_its_single_calls_and_two_runs_are_byte_equal():
    problems = batch()
    merged, counts, _ = run(problems, 0.01)
    again, counts_again, _ = run(problems, 0.01)
    assert cases.same_cloud(again, merged) and np.array_equal(counts, counts_again)
    singles = [run([p], 0.01) for p in problems]
    assert counts.tolist() == [int(s[1][0]) for s in singles]
    assert cases.same_cloud(merged, cases.concatenate([s[0] for s in singles]))
    want = [cases.prune(p["views"], 0.01)[0] for p in problems if len(p["views"])]
    assert cases.same_cloud(merged, cases.concatenate(want))
    assert counts[2] == 0 and counts[4] == 0 and counts[5] == 0 and counts.sum() > 0


def test_zero_problems_and_a_problem_that_keeps_nothing():
    merged, counts, ms = run([], 0.01)
    assert len(counts) == 0 and ms == 0.0 and [a.shape for a in merged] == [(0, 3), (0, 3), (0, 3), (0,)]
    merged, counts, _ = run([cases.problem("zero_first")], 0.01)
    assert counts.tolist() == [0] and [a.shape for a in merged] == [(0, 3), (0, 3), (0, 3), (0,)]


def test_the_block_count_scan_over_several_chunks():
    """640 x 480 is 1 200 pixel blocks of 256; the scan kernel takes 512 block counts per step (kScanChunk of prune.hip), so the running
    row offset is carried over two chunk boundaries.  One view: every live pixel is kept, and the expected rows are the restatement's
    vectorised backprojection of the live pixels in raster order."""
    w, h = 640, 480
    rng = np.random.default_rng(20240611)
    depth = rng.uniform(2.0, 6.0, (h, w)).astype(np.float32)
    depth[rng.random((h, w)) < 0.37] = 0  # about 95 live pixels of a block's 256, another number in every block
    depth[200:203] = 0                    # blocks that keep nothing
    R = cases.rotation(0.02, -0.05, 0.01)
    view = cases.dress([(cases.camera(w, h), R, -R @ np.array([0.1, -0.2, 0.05]), depth)])
    want, tally = cases.prune(view, 0.01)
    live = int(np.count_nonzero(depth > 0))
    assert len(want[3]) == live and np.array_equal(tally["kept"], np.flatnonzero(depth.reshape(-1) > 0))
    got, counts, _ = run([{"views": view}], 0.01)
    assert counts.tolist() == [live]
    assert cases.same_cloud(got, want)
    # beside another problem: the offsets of the second problem start where the first one's 1 200 blocks end
    got, counts, _ = run([{"views": view}, cases.problem("t001_behind")], 0.01)
    assert counts.tolist() == [live, len(cases.expected("t001_behind")[0][3])]
    assert cases.same_cloud(got, cases.concatenate([want, cases.expected("t001_behind")[0]]))


def test_refusals():
    from opensfm_amd import _lib, dense

    with pytest.raises(_lib.OsfmError, match="NaN"):
        run([cases.problem("t001_behind")], float("nan"))
    views = cases.problem("t001_behind")["views"]
    bad = list(views)
    bad[1] = (np.full((3, 3), np.inf),) + views[1][1:]
    with pytest.raises(_lib.OsfmError, match="not finite"):
        run([{"views": bad}], 0.01)
    with pytest.raises(_lib.OsfmError, match="more than 32"):
        run([{"views": [views[0]] * 33}], 0.01)
    for k, name in ((4, "plane"), (5, "color"), (6, "label")):
        bad = list(views)
        bad[1] = views[1][:k] + (views[1][k][:-1],) + views[1][k + 1:]
        with pytest.raises(ValueError, match=f"depth and {name} must have matching shapes"):
            run([{"views": bad}], 0.01)
    # buffers one row short of what the batch keeps: refused, the counts filled in, the buffers untouched
    problems = batch()
    _, counts, _ = run(problems, 0.01)
    capacity = int(counts.sum()) - 1
    offsets, (K, R, t), (depths, planes, colors, labels), widths, heights = dense._pack_prune_views(problems)
    params = dense.params_from_config({"depthmap_same_depth_threshold": 0.01})
    out = (np.full((capacity, 3), 7, np.float32), np.full((capacity, 3), 7, np.float32), np.full((capacity, 3), 7, np.uint8), np.full(capacity, 7, np.uint8))
    got_counts = np.full(len(problems), -1, np.int64)
    status = _lib.load().osfm_depthmap_prune(
        _lib.default_context().handle, len(problems), dense._dptr(offsets, C.c_int32), dense._dptr(K, C.c_double), dense._dptr(R, C.c_double),
        dense._dptr(t, C.c_double), dense._pointers(depths), dense._pointers(planes), dense._pointers(colors), dense._pointers(labels),
        dense._dptr(widths, C.c_int32), dense._dptr(heights, C.c_int32), C.byref(params), C.c_int64(capacity), dense._dptr(out[0], C.c_float),
        dense._dptr(out[1], C.c_float), dense._dptr(out[2], C.c_uint8), dense._dptr(out[3], C.c_uint8), dense._dptr(got_counts, C.c_int64), None)
    assert status == -1 and b"rows" in _lib.load().osfm_last_error()  # OSFM_E_INVALID
    assert np.array_equal(got_counts, counts) and all((a == 7).all() for a in out)
    merged, counts_after, _ = run(problems, 0.01)  # the context is as good as before
    assert np.array_equal(counts_after, counts)


def test_compat_pruner_and_merge_as_dense_py_drives_them():
    """dense.prune_depthmap: a DepthmapPruner, set_same_depth_threshold(config), add_view per neighbour, prune(); dense.merge_depthmaps
    concatenates what the shots gave"""
    from opensfm_amd import dense
    from opensfm_amd.compat import pydense_full

    config = {"depthmap_same_depth_threshold": 0.01}
    names = ("t001_behind", "five_views", "zero_first", "t001_front")
    per_shot = []
    for name in names:
        dp = pydense_full.DepthmapPruner()
        dp.set_same_depth_threshold(config["depthmap_same_depth_threshold"])
        for view in cases.problem(name)["views"]:
            dp.add_view(*view)
        points, normals, colors, labels = dp.prune()
        assert cases.same_cloud((points, normals, colors, labels), cases.expected(name)[0])
        per_shot.append((points, normals, colors, labels))
    assert [a.shape for a in per_shot[2]] == [(0, 3), (0, 3), (0, 3), (0,)]
    problems = [cases.problem(name) for name in names]
    split = dense.prune_depthmaps_arrays(problems, config)
    assert len(split) == len(names) and all(cases.same_cloud(a, b) for a, b in zip(split, per_shot))
    merged = dense.merge_depthmaps_arrays(problems, config)
    assert cases.same_cloud(merged, cases.concatenate(per_shot))
    assert all(a.shape == (0,) for a in dense.merge_depthmaps_arrays([], config))
