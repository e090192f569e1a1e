"""HAHOG extraction on the GPU (csrc/hahog.hip) on the images of ``tests/hahog_cases.py`` -- tied scores under ``target_num_features``, more
orientation peaks than are kept, every step of the octave count, grey levels outside [0, 1], plateaus, padded patches -- against records of
the REFERENCE's features::hahog (tests/golden/hahog_adversarial.npz, made by tests/golden/make_hahog_adversarial_golden.py; the premises
that the cases are what they are taken for are asserted on the reference in tests/test_hahog_cases_host.py).

Stated tolerance: the one at the top of ``test_gpu_hahog.py``.  Row count, order, x, y, size and all 128 descriptor values are the
reference's bit for bit (SHA-256 of the bytes); |angle difference| <= 1e-4 degrees (atan2f's last bit).  Where a hash differs and the
compiled reference is at hand it is run again and the differing rows are counted as ``test_gpu_hahog._compare`` does; the test reads
nothing outside the repository and never skips."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hahog_cases as hc
from opensfm_amd import features
from test_gpu_hahog import _compare

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hahog_adversarial.npz")
OSFM_E_INVALID = -1  # include/osfm_mi355.h


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


def _reference(cid, levels):
    try:
        return hc.reference_levels(cid) if levels else hc.reference(cid)
    except (OSError, subprocess.CalledProcessError):  # no compiled reference and no way to build one here: the hashes are the verdict
        return None


def _check(golden, cid, pts, desc, levels=False, combo=None):
    """(pts, desc) of the library against the records of case ``cid`` (``levels``: of the image features.extract_features_hahog forms;
    ``combo``: descriptors post-processed with that (feature_root, hahog_normalize_to_uchar))"""
    key = cid + ("/levels/" if levels else "/")
    desc_key = key + (hc.combo_key(*combo) if levels else "desc_sha")
    n = int(golden[key + "n"])
    assert pts.dtype == np.float32 and desc.dtype == np.float32 and pts.shape[1:] == (4,) and desc.shape[1:] == (128,)
    got = (hc.sha(pts[:, :3]), hc.sha(desc))
    want = (str(golden[key + "pts_sha"]), str(golden[desc_key]))
    print("%s%s: %d rows (reference %d)" % (cid, " %s" % (combo,) if levels else "", len(pts), n))
    if len(pts) != n or got != want:
        ref = _reference(cid, levels)
        if ref is not None:
            rp, rd = ref
            _compare(pts, desc, rp, hc.postprocess(rd, *combo) if levels else rd)
        pytest.fail("%s: %d rows, reference %d; keypoint hash %s, reference %s; descriptor hash %s, reference %s" % ((cid, len(pts), n, got[0], want[0], got[1], want[1])))
    if n:
        dang = np.abs(pts[:, 3] - golden[key + "angle"])
        dang = np.minimum(dang, 360.0 - dang)
        assert dang.max() <= 1e-4, (cid, dang.max())


@pytest.mark.parametrize("cid", hc.CASE_IDS)
def test_every_case_equals_the_reference(gpu_ctx, golden, cid):
    _, im, peak, edge, target = hc.case(cid)
    pts, desc = features.hahog(hc.float_image(im), peak, edge, target, ctx=gpu_ctx)
    _check(golden, cid, pts, desc)
    if cid in hc.EMPTY_IDS:
        assert pts.shape == (0, 4) and desc.shape == (0, 128)


@pytest.mark.parametrize("cid", hc.COMBO_CASES)
def test_descriptor_post_processing_combinations(gpu_ctx, golden, cid):
    """features.extract_features_hahog with feature_root x hahog_normalize_to_uchar: the reference's float descriptors through
    opensfm/features.py:526-534 in numpy (np.sqrt, x 362 or x 512, clip, round).  ``edge_blobs`` is where x 512 passes 255"""
    _, im, peak, edge, target = hc.case(cid)
    levels, _ = hc.levels_image(im)
    assert levels.dtype == np.float64
    for root, uchar in hc.COMBOS:
        cfg = {"feature_root": root, "hahog_normalize_to_uchar": uchar, "hahog_peak_threshold": peak, "hahog_edge_threshold": edge}
        pts, desc = features.extract_features_hahog(levels, cfg, target, ctx=gpu_ctx)
        _check(golden, cid, pts, desc, levels=True, combo=(root, uchar))
        if uchar:
            assert np.array_equal(desc, np.round(desc)) and desc.min() >= 0 and desc.max() <= 255
            if cid.startswith("edge_blobs") and not root:
                assert (desc == 255).any()


def _bytes_image(im):
    return np.ascontiguousarray(np.round(np.clip(im, 0, 1) * 255), np.uint8)


@pytest.mark.parametrize("cid", hc.U8_CASES)
def test_uint8_images_equal_their_float_form(gpu_ctx, golden, cid):
    """OSFM_HAHOG_IMAGE_U8 on plateaus of 0 and 255: level / 255 formed on the device equals image.astype(np.float32) / 255 byte for byte"""
    _, im, peak, edge, target = hc.case(cid)
    u8 = _bytes_image(im)
    pf, df = features._extract(u8.astype(np.float32) / 255, peak, edge, target, 0, gpu_ctx)
    pu, du = features._extract(u8, peak, edge, target, features.HAHOG_IMAGE_U8, gpu_ctx)
    assert len(pf) >= 5 and pf.tobytes() == pu.tobytes() and df.tobytes() == du.tobytes()
    if np.array_equal(u8.astype(np.float32) / 255, im):  # the images of 0 and 1: the bytes are the case itself
        _check(golden, cid, pu, du)
    else:
        assert cid.startswith("saturated")


def test_constant_uint8_images_have_no_features(gpu_ctx):
    cfg = {"feature_root": True, "hahog_normalize_to_uchar": True, "hahog_peak_threshold": hc.PEAK, "hahog_edge_threshold": hc.EDGE}
    for v in (0, 128, 255):
        im = hc.image("u8_%d" % v)
        assert im.dtype == np.uint8 and im.shape == (64, 80) and (im == v).all()
        for pts, desc in (features._extract(im, hc.PEAK, hc.EDGE, hc.ALL, features.HAHOG_IMAGE_U8, gpu_ctx), features.extract_features_hahog(im, cfg, 500, ctx=gpu_ctx)):
            assert pts.shape == (0, 4) and desc.shape == (0, 128)
    for (pts, desc) in features.hahog_batch([hc.image("u8_%d" % v) for v in (0, 128, 255)], hc.PEAK, hc.EDGE, 500, ctx=gpu_ctx):
        assert pts.shape == (0, 4) and desc.shape == (0, 128)


def _resident_sets():
    """two float images and two byte images, with the flag their kind needs beside OSFM_HAHOG_IMAGE_ON_DEVICE"""
    return (([hc.image("periodic"), hc.image("oct121")], 0),
            ([_bytes_image(hc.image("checker8")), _bytes_image(hc.image("saturated"))], features.HAHOG_IMAGE_U8))


def check_resident_images(ctx, upload, golden_check):
    """OSFM_HAHOG_IMAGE_ON_DEVICE: ``upload(image)`` -> (device address, an object that keeps the copy alive); the addresses go through
    hahog_batch(shapes=...) and every result equals the host-image call byte for byte"""
    target = 333
    fl = features.HAHOG_ROOT | features.HAHOG_UCHAR
    for ims, extra in _resident_sets():
        host = features.hahog_batch(ims, hc.PEAK, hc.EDGE, target, fl, concurrency=2, ctx=ctx)
        dev = [upload(im) for im in ims]  # kept alive until the calls have returned
        got = features.hahog_batch([a for a, _ in dev], hc.PEAK, hc.EDGE, target, fl | extra, concurrency=2, shapes=[im.shape for im in ims], ctx=ctx)
        assert len(got) == len(host) == 2
        for (p, d), (ph, dh) in zip(got, host):
            assert len(p) > 100 and p.tobytes() == ph.tobytes() and d.tobytes() == dh.tobytes()
        if not extra:  # the resident image without post-processing: the golden record of periodic at this target
            raw = features.hahog_batch([dev[0][0]], hc.PEAK, hc.EDGE, target, 0, shapes=[ims[0].shape], ctx=ctx)
            golden_check("periodic@333", *raw[0])
        del dev


def test_device_resident_images_equal_host_images(gpu_ctx, golden):
    """resident copies made with the HIP runtime the library runs on (hipMalloc + hipMemcpy, as bench.py does)"""
    hip = C.CDLL("libamdhip64.so")
    held = []

    def upload(im):
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(im.nbytes)) == 0
        held.append(d)
        assert hip.hipMemcpy(d, C.c_void_p(im.ctypes.data), C.c_size_t(im.nbytes), 1) == 0  # hipMemcpyHostToDevice, done on return
        return d.value, d

    try:
        check_resident_images(gpu_ctx, upload, lambda cid, p, d: _check(golden, cid, p, d))
    finally:
        for d in held:
            assert hip.hipFree(d) == 0


def test_device_resident_torch_tensors_equal_host_images():
    """the same with torch tensors' data_ptr().  A fresh interpreter: torch has to bring up its HIP runtime before the library is loaded
    (as in bench.py and tests/test_gpu_dist.py), which the earlier tests of this pytest process have already prevented"""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hahog_torch_resident_check.py")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "resident torch tensors OK: 4 images" in r.stdout


def _batch_order():
    """every case below one megapixel once, large and small alternating, the image without features in the middle"""
    names = [n for n in dict.fromkeys(c.split("@")[0] for c in hc.CASE_IDS) if n not in ("big8", "checker4")]
    names.sort(key=lambda n: -hc.image(n).size)
    half = (len(names) + 1) // 2
    order = [n for pair in zip(names[:half], names[::-1][:half]) for n in pair][: len(names)]
    assert sorted(order) == sorted(names)
    order.insert((len(order) + 1) // 2, "checker4")
    return order


def test_batch_of_every_case_equals_image_by_image(gpu_ctx, golden):
    order = _batch_order()
    assert len(order) >= 25 and order[len(order) // 2] == "checker4" and "oct961" in order[:2] and "oct17" in order[:2]
    ims = [hc.float_image(hc.image(n)) for n in order]
    target = 333
    single = [features._extract(im, hc.PEAK, hc.EDGE, target, 0, gpu_ctx) for im in ims]
    single = [(p.copy(), d.copy()) for p, d in single]
    _check(golden, "periodic@333", *single[order.index("periodic")])
    assert len(single[order.index("checker4")][0]) == 0 and sum(len(p) for p, _ in single) > 3000
    for conc in (1, 3, 8):
        got = features.hahog_batch(ims, hc.PEAK, hc.EDGE, target, 0, concurrency=conc, ctx=gpu_ctx)
        assert len(got) == len(single)
        for name, (p, d), (ps, ds) in zip(order, got, single):
            assert p.tobytes() == ps.tobytes() and d.tobytes() == ds.tobytes(), (name, conc)


def test_capacity_edge_of_the_c_entry_point(gpu_ctx, golden):
    """osfm_hahog_extract with room for exactly the n rows there are succeeds; with n - 1 it returns OSFM_E_INVALID, reports n, and the
    context works afterwards"""
    from opensfm_amd import _lib

    lib = _lib.load()
    cid = "checker8@150"
    _, im, peak, edge, target = hc.case(cid)
    n = int(golden[cid + "/n"])
    assert 150 < n < 4 * 150

    def call(cap):
        pts, desc = np.full((cap + 1, 4), -7.0, np.float32), np.full((cap + 1, 128), -7.0, np.float32)
        nf = C.c_int(-1)
        rc = lib.osfm_hahog_extract(gpu_ctx.handle, im.ctypes.data_as(C.POINTER(C.c_float)), im.shape[0], im.shape[1], peak, edge, target, 0,
                                    pts.ctypes.data_as(C.POINTER(C.c_float)), desc.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(nf))
        assert (pts[cap] == -7.0).all() and (desc[cap] == -7.0).all()  # nothing past the capacity
        return rc, nf.value, pts[:cap], desc[:cap]

    rc, nf, pts, desc = call(n)
    assert rc == 0 and nf == n
    _check(golden, cid, pts, desc)
    rc, nf, pts, desc = call(n - 1)
    assert rc == OSFM_E_INVALID and nf == n and b"capacity" in lib.osfm_last_error()
    with pytest.raises(_lib.OsfmError):
        _lib.check(rc, "osfm_hahog_extract")
    pts, desc = features.hahog(im, peak, edge, target, ctx=gpu_ctx)
    _check(golden, cid, pts, desc)


@pytest.mark.parametrize("cid", ["periodic@333", "blob0@%d" % hc.ALL])
def test_two_runs_are_byte_equal(gpu_ctx, cid):
    _, im, peak, edge, target = hc.case(cid)
    a = [x.copy() for x in features.hahog(im, peak, edge, target, ctx=gpu_ctx)]
    b = features.hahog(im, peak, edge, target, ctx=gpu_ctx)
    assert len(a[0]) >= 5 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
