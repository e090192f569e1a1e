"""osfm_camera_mapping / osfm_remap_images / osfm_undistort_images / osfm_panorama_mapping on the GPU against the plain restatement of
tests/undistort_cases.py: remap byte for byte, the camera mapping bit for bit (one float32 ulp for the models that call atan / sin / cos),
the fused path byte-equal to map-then-remap, batches against single calls, a panorama into six views, and ``undistort_image`` /
``undistort_images`` called the way ``undistort_image_and_masks`` calls them.  The restatement's results are the stored ones of
tests/golden/undistort (tests/test_undistort_host.py regenerates and compares them)."""
import itertools

import numpy as np
import pytest

import undistort_cases as cases

pytestmark = pytest.mark.gpu

FRAME_MODELS = ("perspective", "brown", "fisheye", "fisheye_opencv", "fisheye62")


def camera(model, par, width=0, height=0, cid=""):
    from opensfm_amd.geometry_types import Camera, set_camera_parameter_values

    c = Camera(model)
    set_camera_parameter_values(c, par)
    c.id, c.width, c.height = cid, width, height
    return c


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def mapping_distance(got, want):
    return max(int(cases.ulp_distance(g, w).max()) for g, w in zip(got, want))


@pytest.mark.parametrize("mode", list(cases.MODES))
@pytest.mark.parametrize("name", list(cases.REMAP_CASES))
def test_remap_is_byte_equal_to_the_restatement(name, mode):
    from opensfm_amd import undistort

    src, map1, map2 = cases.remap_case(name)
    interpolation, border = cases.MODES[mode]
    got = undistort.remap(src, map1, map2, interpolation, border)
    want = cases.load("remap_" + name)[mode]
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"
    if interpolation == cases.INTER_LINEAR:
        assert np.array_equal(undistort.remap(src, map1, map2, undistort.INTER_AREA, border), want)


@pytest.mark.parametrize("size", cases.MAPPING_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mapping_of_every_model_equals_the_restatement(size):
    from opensfm_amd import undistort

    width, height = size
    stored = cases.load(f"mapping_{width}x{height}")
    names = cases.mapping_names(width, height)
    assert set(cases.CAMERAS) <= set(names) and len(cases.CAMERAS) == 10
    pairs = [(camera(*cases.MAPPING_CASES[n][0]), camera(*cases.MAPPING_CASES[n][1]), width, height) for n in names]
    maps, _ = undistort.compute_camera_mappings(pairs)
    outside = 0
    for n, got in zip(names, maps):
        worst = mapping_distance(got, (stored[n + "_map1"], stored[n + "_map2"]))
        print(f"{n}: {worst} float32 ulp")
        assert got[0].dtype == np.float32 and got[0].shape == (height, width)
        assert worst <= (0 if cases.mapping_is_exact(n) else 1), (n, worst)
        outside += bool((got[0] < -1).any() or (got[0] > width).any())
    assert outside >= 6
    alone = undistort.compute_camera_mapping(*pairs[2])
    assert same_bits(alone[0], maps[2][0]) and same_bits(alone[1], maps[2][1])


@pytest.mark.parametrize("width,height,focal", [(64, 64, 0.5), (64, 32, 0.5), (32, 64, 1.0), (128, 64, 2.0)])
def test_identity_mapping_is_the_pixel_grid_exactly(width, height, focal):
    """power-of-two sizes and focals, at which every step of the double chain that touches column 0 and row 0 is exact
    (tests/test_undistort_host.py gives the reasoning): the grid in every entry, and the image back byte for byte"""
    from opensfm_amd import undistort

    cam = camera("perspective", [0.0, 0.0, focal], width, height, "c")
    new = undistort.perspective_camera_from_perspective(cam)
    map1, map2 = undistort.compute_camera_mapping(cam, new, width, height)
    v, u = np.indices((height, width))
    assert np.array_equal(map1, u.astype(np.float32)) and np.array_equal(map2, v.astype(np.float32))
    image = np.random.default_rng(3).integers(0, 256, (height, width, 3), dtype=np.uint8)
    for interpolation in (undistort.INTER_AREA, undistort.INTER_NEAREST):
        out, _ = undistort.undistort_raw([image], [0], [cam], [new], interpolation)
        assert np.array_equal(out[0], image)


@pytest.mark.parametrize("model", FRAME_MODELS)
def test_fused_undistortion_equals_remap_of_the_camera_mapping(model):
    """pins the fused kernel without a tolerance on pixels; the device map is within the mapping tolerance of the restatement, and the
    restatement's remap of the DEVICE map gives the same bytes"""
    from opensfm_amd import undistort

    rng = np.random.default_rng(FRAME_MODELS.index(model))
    cam = camera(model, cases.CAMERAS[model], 65, 33, "c")
    new = undistort.undistorted_camera(cam)
    assert new.focal == cases.undistorted_focal(model, cases.CAMERAS[model])
    for shape in ((33, 65, 3), (48, 64), (70, 130, 4)):
        image = rng.integers(0, 256, shape, dtype=np.uint8)
        h, w = shape[:2]
        map1, map2 = undistort.compute_camera_mapping(cam, new, w, h)
        if (w, h) in cases.MAPPING_SIZES:
            stored = cases.load(f"mapping_{w}x{h}")
            assert mapping_distance((map1, map2), (stored[model + "_map1"], stored[model + "_map2"])) <= (0 if cases.mapping_is_exact(model) else 1)
        for interpolation in (undistort.INTER_AREA, undistort.INTER_NEAREST):
            fused, _ = undistort.undistort_raw([image], [0], [cam], [new], interpolation)
            assert np.array_equal(fused[0], undistort.remap(image, map1, map2, interpolation))
            if shape == (33, 65, 3):
                assert np.array_equal(fused[0], cases.remap(image, map1, map2, interpolation))
                assert (fused[0] == 0).all(axis=2).any() and fused[0].any()  # the corners read outside the source
            scaled, _ = undistort.undistort_raw([image], [0], [cam], [new], interpolation, [cases.scale_size(h, w, 40)])
            assert np.array_equal(scaled[0], undistort.remap(image, map1, map2, interpolation, out_size=cases.scale_size(h, w, 40)))
            if shape == (33, 65, 3):
                assert np.array_equal(scaled[0], cases.scale_image(fused[0], 40))


def test_a_batch_equals_its_single_calls_and_two_runs_agree():
    from opensfm_amd import undistort

    rng = np.random.default_rng(41)
    images = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((29, 37, 3), (33, 65), (70, 130, 4), (1, 1))]
    froms = [camera(m, cases.CAMERAS[m]) for m in ("brown", "fisheye62")]
    tos = [undistort.undistorted_camera(c) for c in froms]
    cam_of = [0, 1, 1, 0]
    sizes = [None, (20, 40), None, None]
    for interpolation in (undistort.INTER_AREA, undistort.INTER_NEAREST):
        together, _ = undistort.undistort_raw(images, cam_of, froms, tos, interpolation, sizes)
        again, _ = undistort.undistort_raw(images, cam_of, froms, tos, interpolation, sizes)
        maps = [undistort.compute_camera_mapping(froms[c], tos[c], im.shape[1], im.shape[0]) for im, c in zip(images, cam_of)]
        remapped, _ = undistort.remap_raw(images, maps, interpolation, undistort.BORDER_CONSTANT, sizes)
        shared, _ = undistort.remap_raw([images[0], images[0]], [maps[0], maps[0]], interpolation)  # one map, uploaded once
        assert np.array_equal(shared[0], shared[1]) and np.array_equal(shared[0], together[0])
        for k, image in enumerate(images):
            alone, _ = undistort.undistort_raw([image], [0], [froms[cam_of[k]]], [tos[cam_of[k]]], interpolation, [sizes[k]])
            assert np.array_equal(together[k], alone[0]) and np.array_equal(together[k], again[k]) and np.array_equal(together[k], remapped[k])
    assert undistort.undistort_raw([], [], froms, tos, undistort.INTER_AREA) == ([], 0.0)
    assert undistort.remap_raw([], [], undistort.INTER_LINEAR) == ([], 0.0)
    assert undistort.compute_camera_mappings([]) == ([], 0.0)
    assert undistort.panorama_mappings(camera("spherical", []), [], 128, 64) == ([], 0.0)


def panorama_scene(undistort):
    from opensfm_amd.geometry_types import Pose, Reconstruction

    rec, urec = Reconstruction(), Reconstruction()
    rec.add_camera(camera("spherical", [], 2048, 1024, "pano"))
    pose = Pose()
    pose.set_rotation_matrix(cases.panorama_pose_rotation())
    shot = rec.create_shot("pano.jpg", "pano", pose)
    return shot, undistort.perspective_views_of_a_panorama(shot, cases.PANORAMA["view"], urec, "jpg", itertools.count())


def test_panorama_into_six_views():
    from opensfm_amd import undistort

    stored, image, R_pano = cases.load("panorama"), cases.panorama_image(), cases.panorama_pose_rotation()
    view_cam = camera("perspective", [0.0, 0.0, 0.5], 32, 32)
    maps, _ = undistort.panorama_mappings(camera("spherical", []), [(view_cam, np.dot(R_pano, R.T)) for R in cases.view_rotations()], 128, 64)
    seam = poles = 0
    for name, (x, y) in zip(cases.VIEW_NAMES, maps):
        worst = mapping_distance((x, y), (stored[name + "_x"], stored[name + "_y"]))
        print(f"{name}: {worst} float32 ulp")
        assert worst <= 1, (name, worst)
        seam += bool((x < 1).any() and (x > 126).any())
        poles += bool((y < 1).any() or (y > 62).any())
        for label in ("linear", "nearest"):  # the restatement's remap of the DEVICE map, byte for byte; and the stored views where the maps agree
            interpolation = cases.MODES[label + "_wrap"][0]
            got = undistort.remap(image, x, y, interpolation, "wrap")
            assert np.array_equal(got, cases.remap(image, x, y, interpolation, cases.BORDER_WRAP))
            if worst == 0:
                assert np.array_equal(got, stored[name + "_" + label])
    assert seam >= 1 and poles >= 2  # BORDER_WRAP across the +-pi seam and at the poles
    shot, views = panorama_scene(undistort)
    assert [v.id for v in views] == [f"pano.jpg_perspective_view_{n}.jpg" for n in cases.VIEW_NAMES]
    own, _ = undistort.panorama_mappings(shot.camera, [(v.camera, undistort._view_rotation(shot, v)) for v in views], 128, 64)
    for interpolation, label in ((undistort.INTER_AREA, "linear"), (undistort.INTER_NEAREST, "nearest")):
        got = undistort.undistort_image(shot, views, image, interpolation, 24)
        assert list(got) == [v.id for v in views]
        for v, (x, y) in zip(views, own):
            want = cases.scale_image(cases.remap(image, x, y, cases.MODES[label + "_wrap"][0], cases.BORDER_WRAP), 24)
            assert got[v.id].shape == (24, 24, 3) and np.array_equal(got[v.id], want)
    with pytest.raises(ValueError):
        undistort.undistort_image(shot, views, image[:, :100], undistort.INTER_AREA, 24)


def test_undistort_image_and_undistort_images_as_the_reference_calls_them():
    from opensfm_amd import undistort
    from opensfm_amd.geometry_types import Reconstruction

    rng = np.random.default_rng(23)
    rec, urec = Reconstruction(), Reconstruction()
    for cid, model in (("a", "brown"), ("b", "fisheye")):
        c = rec.add_camera(camera(model, cases.CAMERAS[model], 64, 48, cid))
        urec.add_camera(undistort.undistorted_camera(c))
    shots = [rec.create_shot(f"im{k}", cid) for k, cid in enumerate("aba")]
    ushots = [urec.create_shot(undistort.add_image_format_extension(s.id, "jpg"), s.camera.id, s.pose) for s in shots]
    images = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8) for _ in shots]
    masks = [rng.integers(0, 2, (48, 64), dtype=np.uint8) * 255, None, rng.integers(0, 2, (48, 64), dtype=np.uint8)]
    segmentations = [None, rng.integers(0, 20, (48, 64), dtype=np.uint8), None]
    max_size = 40  # smaller than the image: scale_image resizes to 40 x 30
    batch = undistort.undistort_images(shots, images, masks, segmentations, max_size)
    stored = cases.load("mapping_64x48")
    for k, shot in enumerate(shots):
        model = shot.camera.projection_type
        lib_map = undistort.compute_camera_mapping(shot.camera, ushots[k].camera, 64, 48)
        assert mapping_distance(lib_map, (stored[model + "_map1"], stored[model + "_map2"])) <= (0 if cases.mapping_is_exact(model) else 1)
        for kind, arrays, interpolation in (("image", images, undistort.INTER_AREA), ("mask", masks, undistort.INTER_NEAREST),
                                            ("segmentation", segmentations, undistort.INTER_NEAREST)):
            one = undistort.undistort_image(shot, [ushots[k]], arrays[k], interpolation, max_size)
            if arrays[k] is None:
                assert one == {} and batch[k][kind] is None
                continue
            want = cases.scale_image(cases.remap(arrays[k], lib_map[0], lib_map[1], interpolation), max_size)
            assert list(one) == [f"im{k}.jpg"] and want.shape[:2] == (30, 40)
            assert np.array_equal(one[f"im{k}.jpg"], want) and np.array_equal(batch[k][kind], want)


def test_refusals_leave_the_outputs_alone():
    import ctypes as C

    from opensfm_amd import _lib, undistort

    cam = camera("brown", cases.CAMERAS["brown"])
    new = undistort.undistorted_camera(cam)
    image = np.full((6, 8, 3), 9, np.uint8)
    map1, map2 = np.zeros((6, 8), np.float32), np.zeros((6, 8), np.float32)
    view = camera("perspective", [0.0, 0.0, 0.5], 8, 8)
    rotation = np.eye(3)
    rotation[2, 0] = float("nan")
    for call, needle in ((lambda: undistort.remap(np.zeros((6, 8, 2), np.uint8), map1, map2, undistort.INTER_LINEAR), "2 channels"),
                         (lambda: undistort.remap(image.astype(np.uint16), map1, map2, undistort.INTER_LINEAR), "uint16"),
                         (lambda: undistort.compute_camera_mapping(cam, new, 32768, 4), "32767"),
                         (lambda: undistort.compute_camera_mapping(cam, new, 0, 4), "not positive"),
                         (lambda: undistort.undistort_raw([image], [1], [cam], [new], undistort.INTER_AREA), "outside the table"),
                         (lambda: undistort.panorama_mappings(camera("spherical", []), [(view, rotation)], 32, 16), "rotation is not finite")):
        with pytest.raises(_lib.OsfmError, match=r"\(-1\)") as e:
            call()
        assert needle in str(e.value)
    broken = camera("brown", cases.CAMERAS["brown"])
    broken.k2 = float("nan")
    with pytest.raises(_lib.OsfmError, match="not finite"):
        undistort.undistort_raw([image], [0], [broken], [new], undistort.INTER_AREA)
    # the C ABI: a refused call leaves the output buffer and kernel_ms as they were; the same call with valid arguments then fills both
    lib, ctx = _lib.load(), _lib.default_context()
    out, ms = np.full((6, 8, 3), 0xA5, np.uint8), C.c_double(-7.0)
    w, h, c, cam_of = np.array([8], np.int32), np.array([6], np.int32), np.array([3], np.int32), np.array([0], np.int32)
    ip, dp, vp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: (C.c_void_p * 1)(a.ctypes.data))
    (fm, fp), (tm, tp) = undistort._camera_table([cam]), undistort._camera_table([new])
    for interpolation, border in ((2, 0), (1, 1), (-1, 0), (1, 4)):
        rc = lib.osfm_remap_images(ctx.handle, 1, vp(image), ip(w), ip(h), ip(c), vp(map1), vp(map2), ip(w), ip(h), ip(w), ip(h), interpolation,
                                   border, vp(out), C.byref(ms))
        assert rc == -1 and (out == 0xA5).all() and ms.value == -7.0 and b"unknown" in lib.osfm_last_error()
    for channels, index in ((2, 0), (3, 1)):
        rc = lib.osfm_undistort_images(ctx.handle, 1, vp(image), ip(w), ip(h), ip(np.array([channels], np.int32)), ip(np.array([index], np.int32)), 1,
                                       ip(fm), dp(fp), ip(tm), dp(tp), ip(w), ip(h), 1, vp(out), C.byref(ms))
        assert rc == -1 and (out == 0xA5).all() and ms.value == -7.0
    rc = lib.osfm_undistort_images(ctx.handle, 1, vp(image), ip(w), ip(h), ip(c), ip(cam_of), 1, ip(fm), dp(fp), ip(tm), dp(tp), ip(w), ip(h), 1,
                                   vp(out), C.byref(ms))
    assert rc == 0 and ms.value >= 0.0 and not (out == 0xA5).all()
