"""osfm_depthmap_estimate / osfm_depthmap_clean on the GPU against the numpy restatement of depthmap.cc (tests/depthmap_cases.py): all four
outputs byte for byte, for the three methods on every shape of ``cases.CASES``; the batch against single calls; the cleaner; refusals; and
``compat.pydense`` called the way opensfm/dense.py calls it.  The restatement's results are the stored ones of tests/golden/depthmap
(tests/test_depthmap_host.py regenerates and compares them) when they were made with the library's tables, else they are computed."""

import numpy as np
import pytest

import depthmap_cases as cases

pytestmark = pytest.mark.gpu

METHODS = (cases.BRUTE_FORCE, cases.PATCH_MATCH, cases.PATCH_MATCH_SAMPLE)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bytes(got, want):
    return all(g.shape == w.shape and g.dtype == w.dtype and np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def params(method, patch_size=5, iterations=1, num_planes=8, **more):
    from opensfm_amd import dense

    return dense.params_from_config(None, method=method, patch_size=patch_size, patchmatch_iterations=iterations, num_depth_planes=num_planes, **more)


@pytest.mark.parametrize("method", METHODS, ids=[cases.METHOD_NAMES[m] for m in METHODS])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_outputs_are_byte_equal_to_the_restatement(name, method):
    from opensfm_amd import dense

    problem = cases.problem(name)
    tables = dense.tables(problem["min_depth"], problem["max_depth"])
    got, ms = dense.estimate_raw([problem], params(method, **cases.CASES[name][1]), cases.SEED)
    want = cases.expected(name, method, tables, tables["init_depth"])
    for k, what in enumerate(("depth", "plane", "score", "nghbr")):
        differ = int((bits(got[0][k]) != bits(want[k])).sum())
        assert got[0][k].dtype == want[k].dtype and differ == 0, f"{what}: {differ} of {want[k].size} entries differ"
    if name == "below_patch":
        assert ms == 0.0 and not any(a.any() for a in got[0])  # zeros, no launch
    if name == "single_view":  # no candidate is ever scored in a view
        if method == cases.BRUTE_FORCE:
            assert not any(a.any() for a in got[0])  # -1 never exceeds the initial 0: all-zero
        else:
            assert (got[0][0] != 0).any() and (got[0][2][got[0][0] != 0] == -1).all() and not got[0][3].any()
    if name == "all_outside":  # the last view's samples all lie outside its (non-zero) image: it scores -1 and is never the neighbour
        assert problem["views"][2][3].any()
        if method != cases.PATCH_MATCH_SAMPLE:
            assert not (got[0][3] == 2).any() and (got[0][3] == 1).any()
        else:
            assert (got[0][2][got[0][3] == 2] == -1).all()
    if name == "duplicate_view" and method != cases.PATCH_MATCH_SAMPLE:
        assert not (got[0][3] == 2).any()  # the repeated view ties with view 1 everywhere: the lower index wins


@pytest.mark.parametrize("method", METHODS, ids=[cases.METHOD_NAMES[m] for m in METHODS])
def test_a_batch_equals_its_single_calls_and_two_runs_agree(method):
    from opensfm_amd import dense

    batch = [cases.problem("other_sizes"), cases.problem("duplicate_view"), {"views": [], "min_depth": 1.0, "max_depth": 2.0},
             dict(cases.problem("one_plane"), min_depth=3.5, max_depth=6.0)]
    p = params(method, patch_size=5, iterations=1, num_planes=8)
    together, _ = dense.estimate_raw(batch, p, 77)
    again, _ = dense.estimate_raw(batch, p, 77)
    for b, problem in enumerate(batch):
        alone, _ = dense.estimate_raw([problem], p, 77)
        assert same_bytes(together[b], alone[0]), f"problem {b} differs between the batch and its single call"
        assert same_bytes(together[b], again[b]), f"problem {b} differs between two runs"
    assert together[2][0].shape == (0, 0)
    assert dense.estimate_raw([], p, 77) == ([], 0.0) and dense.clean_raw([], p) == ([], 0.0)  # a batch of zero problems
    if method != cases.BRUTE_FORCE:
        other, _ = dense.estimate_raw(batch, p, 78)
        assert not same_bytes(together[0], other[0])  # the seed matters


@pytest.mark.parametrize("min_consistent", (1, 2, 3))
def test_the_cleaner_is_byte_equal(min_consistent):
    from opensfm_amd import dense

    problem = cases.clean_problem(n_views=4, behind=True)
    p = params(cases.PATCH_MATCH, same_depth_threshold=0.01, min_consistent_views=min_consistent)
    small = {"views": problem["views"][:2]}
    got, _ = dense.clean_raw([problem, {"views": []}, small], p)
    for g, pr in ((got[0], problem), (got[2], small)):
        want = cases.clean(pr["views"], 0.01, min_consistent)
        assert np.array_equal(bits(g), bits(want))
        assert not g[::5, ::7].any()
    if min_consistent == 1:  # every view is consistent with itself
        assert np.array_equal(bits(got[0]), bits(problem["views"][0][3]))
    else:  # the view behind the camera never agrees, the zeros and the scaled block of view 1 never do
        assert 0 < (got[0] != 0).sum() < (problem["views"][0][3] != 0).sum()
    alone, _ = dense.clean_raw([small], p)
    assert np.array_equal(bits(alone[0]), bits(got[2]))


def test_bad_arguments_are_refused():
    from opensfm_amd import _lib, dense

    good = cases.problem("one_plane")

    def refused(problem=good, **kw):
        with pytest.raises(_lib.OsfmError, match=r"\(-1\)"):
            dense.estimate_raw([problem], params(cases.PATCH_MATCH, **kw), 1)

    refused(patch_size=4)
    refused(patch_size=1)
    refused(patch_size=17)
    refused(num_planes=0)
    refused(dict(good, min_depth=0.0))
    refused(dict(good, min_depth=2.0, max_depth=1.0))
    refused(dict(good, views=good["views"] * 11))  # 33 views
    K, R, t, image, mask = good["views"][1]
    for bad in ((K * np.nan, R, t), (K, R + np.inf, t), (K, R, t * np.nan)):
        refused(dict(good, views=[good["views"][0], bad + (image, mask)]))
    with pytest.raises(ValueError, match="matching shapes"):
        dense.estimate_raw([dict(good, views=[(K, R, t, image, mask[:-1])])], params(cases.PATCH_MATCH), 1)
    with pytest.raises(_lib.OsfmError, match=r"\(-1\)"):
        dense.clean_raw([{"views": [(K * np.nan, R, t, np.ones((4, 4), np.float32))]}], params(cases.PATCH_MATCH))
    # sixteen views are within the limit
    got, _ = dense.estimate_raw([dict(good, views=[good["views"][0]] + [good["views"][1]] * 15)], params(cases.BRUTE_FORCE), 1)
    assert got[0][0].any()


def test_compat_pydense_as_the_reference_calls_it():
    """opensfm/dense.py:114-126 and 185-189"""
    from opensfm_amd import compat, dense

    problem = cases.problem("tall_3views_p5")
    config = {"depthmap_patchmatch_iterations": 1, "depthmap_patch_size": 5, "depthmap_min_patch_sd": 1.0, "depthmap_method": "PATCH_MATCH_SAMPLE",
              "depthmap_min_correlation_score": 0.1, "depthmap_same_depth_threshold": 0.01, "depthmap_min_consistent_views": 2}
    results = {}
    for method in ("BRUTE_FORCE", "PATCH_MATCH", "PATCH_MATCH_SAMPLE"):
        de = compat.pydense.DepthmapEstimator()
        de.set_depth_range(problem["min_depth"], problem["max_depth"], 100)
        de.set_patchmatch_iterations(config["depthmap_patchmatch_iterations"])
        de.set_patch_size(config["depthmap_patch_size"])
        de.set_min_patch_sd(config["depthmap_min_patch_sd"])
        for K, R, t, image, mask in problem["views"]:
            de.add_view(K, R, t, image, mask)
        if method == "BRUTE_FORCE":
            depth, plane, score, nghbr = de.compute_brute_force()
        elif method == "PATCH_MATCH":
            depth, plane, score, nghbr = de.compute_patch_match()
        else:
            depth, plane, score, nghbr = de.compute_patch_match_sample()
        h, w = problem["views"][0][3].shape
        assert (depth.shape, plane.shape, score.shape, nghbr.shape) == ((h, w), (h, w, 3), (h, w), (h, w))
        assert (depth.dtype, plane.dtype, score.dtype, nghbr.dtype) == (np.float32, np.float32, np.float32, np.int32)
        results[method] = (depth, plane, score, nghbr)
    assert de.seed == dense.DEFAULT_SEED
    # the arrays call gives the same, with the reference's two filters applied to the depth
    d, pl, s, n = dense.compute_depthmaps_arrays([problem], config)[0]
    raw = results["PATCH_MATCH_SAMPLE"]
    assert same_bytes((pl, s, n), raw[1:]) and np.array_equal(d, raw[0] * (raw[0] < problem["max_depth"]) * (raw[2] > 0.1))
    with pytest.raises(ValueError, match="matching shapes"):
        de.add_view(np.eye(3), np.eye(3), np.zeros(3), np.zeros((4, 5), np.uint8), np.zeros((5, 4), np.uint8))
    clean_problem = cases.clean_problem(n_views=3, behind=False)
    dc = compat.pydense.DepthmapCleaner()
    dc.set_same_depth_threshold(config["depthmap_same_depth_threshold"])
    dc.set_min_consistent_views(config["depthmap_min_consistent_views"])
    for K, R, t, depth in clean_problem["views"]:
        dc.add_view(K, R, t, depth)
    cleaned = dc.clean()
    assert cleaned.dtype == np.float32 and np.array_equal(bits(cleaned), bits(cases.clean(clean_problem["views"], 0.01, 2)))
    assert 0 < (cleaned != 0).sum() < (clean_problem["views"][0][3] != 0).sum()
    assert np.array_equal(bits(dense.clean_depthmaps_arrays([clean_problem], config)[0]), bits(cleaned))
