"""The cases of ``tests/hahog_cases.py`` on the CPU: every one through the REFERENCE's features::hahog (oracle.hahog_ref, compiled from the
reference checkout), the premises that make ``test_gpu_hahog_adversarial.py`` mean what it says asserted on the reference's results alone,
and the committed golden records (tests/golden/hahog_adversarial.npz) equal to what the reference returns now."""
import os

import numpy as np
import pytest

import hahog_cases as hc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hahog_adversarial.npz")
SKIP = "oracle/_ref/libhahog_ref.so is not available (it is built where /root/reference is mounted)"


def _ref(cid):
    ref = hc.reference(cid)
    if ref is None:
        pytest.skip(SKIP)
    return ref


def test_cases_are_listed_once_and_well_formed():
    assert len(set(hc.CASE_IDS)) == len(hc.CASE_IDS)
    for name, im, peak, edge, target in hc.cases():
        assert im.ndim == 2 and im.flags.c_contiguous and im.dtype == (np.uint8 if name.startswith("u8_") else np.float32), name
        assert peak > 0 and edge > 0 and target > 0
        assert im.size < 1 << 20 or name == "big8"  # the only case above one megapixel
    assert set(hc.COMBO_CASES) | set(hc.U8_CASES) | set(hc.EMPTY_IDS) <= set(hc.CASE_IDS)
    assert hc.case("scaled255@%d" % hc.ALL)[1].max() == 255 and hc.case("shifted@%d" % hc.ALL)[1].min() == -0.5
    assert set(np.unique(hc.case("binary_noise@%d" % hc.ALL)[1])) == {0.0, 1.0}
    sat = hc.case("saturated@%d" % hc.ALL)[1]
    flat = lambda m: int((m[:-2, :-2] & m[:-2, 1:-1] & m[:-2, 2:] & m[1:-1, :-2] & m[1:-1, 1:-1] & m[1:-1, 2:] & m[2:, :-2] & m[2:, 1:-1] & m[2:, 2:]).sum())
    assert flat(sat == 0) >= 100 and flat(sat == 1) >= 100  # plateaus at both ends: 3 x 3 neighbourhoods of equal values


@pytest.mark.parametrize("cid", hc.CASE_IDS)
def test_reference_runs_every_case(cid):
    pts, desc = _ref(cid)
    assert pts.shape == (len(pts), 4) and desc.shape == (len(pts), 128)
    if cid in hc.EMPTY_IDS:
        assert len(pts) == 0
    else:
        assert len(pts) >= 5, len(pts)
        assert np.isfinite(pts).all() and np.isfinite(desc).all()
    target = hc.case(cid)[4]
    assert len(pts) <= 4 * target


@pytest.mark.parametrize("target", hc.PERIODIC_CUT)
def test_periodic_targets_cut_a_group_of_equal_scores(target):
    """some (descriptor, size, angle) row is there j times in the selection and k times in the unlimited run, 0 < j < k: the copies of
    one frame share a score, and which of them survive is the stable sort's decision"""
    full = hc.row_multiset(*_ref("periodic@%d" % hc.ALL))
    sel = hc.row_multiset(*_ref("periodic@%d" % target))
    cut = [(j, full[k]) for k, j in sel.items() if k in full and 0 < j < full[k]]
    print("periodic@%d: %d groups cut, e.g. %s" % (target, len(cut), cut[:4]))
    assert len(cut) >= 1


def test_periodic_has_groups_of_equal_rows():
    full = hc.row_multiset(*_ref("periodic@%d" % hc.ALL))
    assert sum(1 for v in full.values() if v >= 2) >= 100


@pytest.mark.parametrize("name", ["checker6", "checker8"])
def test_checker_corners_carry_four_orientations(name):
    pos = hc.positions(_ref("%s@%d" % (name, hc.ALL))[0])
    four = [a for a in pos.values() if len(a) == 4]
    quarter = [a for a in four if abs(hc.covering_arc(a) - 270.0) < 2.0]
    print(name, "positions with four rows:", len(four), "of which a quarter turn apart:", len(quarter))
    assert len(four) >= 100, len(four)
    n150 = len(_ref("%s@150" % name)[0])
    assert 150 < n150 <= 600  # several rows per selected frame, within the 4 x target rows the binding offers


@pytest.mark.parametrize("name,lo,hi", [("blob6", 0.0, 185.0), ("blob5", 205.0, 225.0)])
def test_blobs_have_more_peaks_than_are_kept(name, lo, hi):
    """six peaks 60 degrees apart of which the first four in bin order span 180 degrees; five peaks 72 degrees apart: 216 degrees.  The
    four largest of six equal peaks, or the last four, would span something else"""
    fr = hc.frames(_ref("%s@%d" % (name, hc.ALL))[0])
    arcs = sorted(hc.covering_arc(a) for a in fr.values() if len(a) == 4)
    print(name, "covering arcs of the four-row frames:", np.round(arcs, 1))
    assert sum(1 for a in arcs if lo <= a <= hi) >= 3, arcs


def test_isotropic_blobs_have_four_row_frames():
    fr = hc.frames(_ref("blob0@%d" % hc.ALL)[0])
    assert sum(1 for a in fr.values() if len(a) == 4) >= 3


@pytest.mark.parametrize("side,n_oct", sorted(hc.OCTAVE_SIDES.items()))
def test_octave_cases_sit_on_the_steps_of_the_octave_count(side, n_oct):
    _, im, _, _, _ = hc.case("oct%d@%d" % (side, hc.ALL))
    assert im.shape == (side, side + 6) and hc.octaves(*im.shape) == n_oct
    assert len(_ref("oct%d@%d" % (side, hc.ALL))[0]) > 0


def test_big_and_thin_octave_counts():
    assert hc.octaves(*hc.case("big8@3000")[1].shape) == 8
    assert hc.octaves(17, 2000) == 1 and hc.octaves(2000, 18) == 1 and hc.octaves(16, 2000) == 0
    assert len(_ref("big8@3000")[0]) > 3000


def test_border_blobs_pad_every_patch():
    _, im, _, _, _ = hc.case("border_blobs@%d" % hc.ALL)
    pts, _ = _ref("border_blobs@%d" % hc.ALL)
    h, w = im.shape
    x, y, size = pts[:, 0], pts[:, 1], pts[:, 2]
    assert len(pts) >= 5
    assert (np.minimum(np.minimum(x, y), np.minimum(w - 1 - x, h - 1 - y)) < 7.5 * size).all()


def test_the_clip_of_the_uchar_scaling_is_active_without_the_root():
    """features.py:526-534: x 512 passes 255 where a descriptor value is above 0.498; x 362 of a square root never does"""
    hit = above = 0
    for cid in hc.COMBO_CASES:
        ref = hc.reference_levels(cid)
        if ref is None:
            pytest.skip(SKIP)
        d = hc.postprocess(ref[1], False, True)
        assert d.max() <= 255 and d.min() >= 0 and np.array_equal(d, np.round(d))
        hit += int((d == 255).sum())
        above += int((512 * ref[1] > 255.5).sum())  # not 255 by rounding: cut by the clip
    print("levels of 255 after x 512: %d, of which %d by the clip" % (hit, above))
    assert hit >= 1 and above >= 1


def test_golden_records_are_what_the_reference_returns_now():
    rec = hc.all_records()
    if rec is None:
        pytest.skip(SKIP)
    g = np.load(GOLDEN)
    assert set(g.files) == set(rec)
    for k, v in rec.items():
        assert g[k].dtype == np.asarray(v).dtype and np.array_equal(g[k], v), k
