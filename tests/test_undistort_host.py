"""Image undistortion on the CPU: the product's undistort.hip compiled for the host against the HIP emulation
(``tests/native/build_undistort_emu.py``) against the plain restatement of ``tests/undistort_cases.py`` -- remap byte for byte, the camera
mapping bit for bit (or to one float32 ulp for the models that call atan / sin / cos); the restated mapping against the reference's own
camera functions where they are compiled; identity, an independent bound on linear interpolation, scaled output, the stand-alone program
under ASan + UBSan, the focal rules, the panorama views and the refusals."""
import contextlib
import ctypes as C
import importlib.util
import itertools
import os
import subprocess

import numpy as np
import pytest

import undistort_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))


def _builder():
    spec = importlib.util.spec_from_file_location("build_undistort_emu", os.path.join(HERE, "native", "build_undistort_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@contextlib.contextmanager
def emulated_undistort():
    """inside: opensfm_amd calls that go through _lib.load() run undistort.hip on the host emulation"""
    from opensfm_amd import _lib

    lib = C.CDLL(_builder().build())
    for name, (res, args) in _lib._signatures().items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    old_lib, old_ctx = _lib._lib, getattr(_lib._tls, "ctx", None)
    _lib._lib, _lib._tls.ctx = lib, {}
    try:
        yield lib
    finally:
        for c in _lib._tls.ctx.values():
            c.close()
        _lib._lib, _lib._tls.ctx = old_lib, old_ctx


@pytest.fixture(scope="module")
def emu():
    with emulated_undistort() as lib:
        yield lib


def camera(model, par):
    """a geometry_types.Camera of `model` with the native parameter vector `par`"""
    from opensfm_amd.geometry_types import Camera, set_camera_parameter_values

    c = Camera(model)
    set_camera_parameter_values(c, par)
    return c


def check_mapping(name, got, want):
    worst = max(int(cases.ulp_distance(g, w).max()) for g, w in zip(got, want))
    print(f"{name}: worst distance {worst} float32 ulp")
    assert all(g.dtype == np.float32 and g.shape == w.shape for g, w in zip(got, want))
    assert worst <= (0 if cases.mapping_is_exact(name) else 1), (name, worst)


# ---- 1. the stored results are the restatement's ----
def test_golden_files_are_what_the_restatement_computes():
    spec = importlib.util.spec_from_file_location("gen_undistort_golden", os.path.join(HERE, "golden", "gen_undistort_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh = {"remap_" + name: gen.remap_results(name) for name in cases.REMAP_CASES}
    fresh.update({f"mapping_{w}x{h}": gen.mapping_results(w, h) for w, h in cases.MAPPING_SIZES})
    fresh["panorama"] = gen.panorama_results()
    for name, arrays in fresh.items():
        stored = cases.load(name)
        assert sorted(stored) == sorted(arrays), name
        for key, value in arrays.items():
            assert stored[key].dtype == value.dtype and np.array_equal(stored[key], value, equal_nan=value.dtype != np.uint8), (name, key)


# ---- 2. the restated mapping against the reference's compiled camera functions ----
@pytest.mark.parametrize("name", [n for n in cases.MAPPING_CASES if cases.MAPPING_CASES[n][0][0] in cases.REF_FORWARD_MODELS])
def test_restated_mapping_equals_the_compiled_reference_cameras(oracle_lib, name):
    """from.Project(to.Bearing(.)) through the reference's own Forward / Backward (oracle/_ref): both sides are double evaluations whose
    error is far below a float32 ulp, so after narrowing they differ by one step at most"""
    if oracle_lib.camera_ref_lib() is None:
        pytest.skip("oracle/_ref/libcamera_ref.so is absent")
    (fm, fp), (tm, tp) = cases.MAPPING_CASES[name]
    width, height = 37, 29
    n = max(width, height)
    v, u = np.indices((height, width))
    px = np.c_[(1.0 / n) * (u.ravel() - width * 0.5), (1.0 / n) * (v.ravel() - height * 0.5)]
    b = oracle_lib.ref_camera(tm, tp, px, backward=True)
    if b is None:
        b = oracle_lib.ref_camera_eigen_backward(tm, tp, px)
        if b is None:
            pytest.skip("oracle/_ref/libcamera_ref_eigen.so is absent")
    p = oracle_lib.ref_camera(fm, fp, b, backward=False)
    assert p is not None, fm
    with np.errstate(over="ignore"):
        want = ((n * p[:, 0] + width * 0.5).astype(np.float32).reshape(height, width), (n * p[:, 1] + height * 0.5).astype(np.float32).reshape(height, width))
    got = cases.camera_mapping((fm, fp), (tm, tp), width, height)
    worst = max(int(cases.ulp_distance(g, w).max()) for g, w in zip(got, want))
    print(f"{name}: restatement against the compiled reference: {worst} float32 ulp")
    assert worst <= 1, (name, worst)


# ---- 3. undistort.hip on the emulation against the restatement ----
@pytest.mark.parametrize("mode", list(cases.MODES))
@pytest.mark.parametrize("name", list(cases.REMAP_CASES))
def test_emulated_remap_is_byte_equal_to_the_restatement(emu, name, mode):
    from opensfm_amd import undistort

    src, map1, map2 = cases.remap_case(name)
    interpolation, border = cases.MODES[mode]
    got = undistort.remap(src, map1, map2, interpolation, border)
    want = cases.load("remap_" + name)[mode]
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"
    if interpolation == cases.INTER_LINEAR:  # INTER_AREA is treated as INTER_LINEAR
        assert np.array_equal(undistort.remap(src, map1, map2, undistort.INTER_AREA, border), want)


def test_remap_cases_hold_what_they_are_meant_to_hold():
    src, map1, map2 = cases.remap_case("37x29")
    fixed = map1[np.isfinite(map1)].astype(np.float64) * 32
    on_tie = np.abs(fixed - np.floor(fixed) - 0.5) == 0
    assert on_tie.sum() >= 8 and np.isnan(map1).any() and np.isinf(map1).any() and (map1 < -1).any() and (map1 == 37).any() and (map1 == 36).any()
    assert (np.abs(map1[np.isfinite(map1)]) > 2 ** 26).any()  # beyond int32 once scaled by 32
    wrap, constant = cases.load("remap_37x29")["linear_wrap"], cases.load("remap_37x29")["linear_constant"]
    assert (wrap != constant).any()


@pytest.mark.parametrize("size", cases.MAPPING_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_emulated_mapping_equals_the_restatement(emu, size):
    from opensfm_amd import undistort

    width, height = size
    stored = cases.load(f"mapping_{width}x{height}")
    names = cases.mapping_names(width, height)
    pairs = [(camera(*cases.MAPPING_CASES[n][0]), camera(*cases.MAPPING_CASES[n][1]), width, height) for n in names]
    maps, _ = undistort.compute_camera_mappings(pairs)  # one batch
    outside = 0
    for n, got in zip(names, maps):
        check_mapping(n, got, (stored[n + "_map1"], stored[n + "_map2"]))
        outside += bool((got[0] < -1).any() or (got[0] > width).any())
    assert outside >= 6  # strong distortion: corners of most cases map outside the source
    alone = undistort.compute_camera_mapping(*pairs[2])
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(alone, maps[2]))


# ---- 4. identity ----
def identity_pair(undistort, width=37, height=29, focal=0.8):
    from opensfm_amd.geometry_types import Camera

    cam = Camera.create_perspective(focal, 0.0, 0.0)
    cam.id, cam.width, cam.height = "c", width, height
    return cam, undistort.perspective_camera_from_perspective(cam)


# sizes and focals at which the identity is exact in EVERY entry, by reasoning: with n = max(w, h) a power of two, h = n, n / 2 or n / 4
# and a power-of-two focal, (1 / n) uv, / focal, * focal and n * are exact, and the undistorted coordinate of column 0 and of row 0,
# x = -(w / 2) / n / focal, is a power of two.  Then x * inv is exact, (x * inv) / inv is x exactly (a correctly rounded quotient of
# exact operands), and n * focal * x + w / 2 is 0 exactly.  Every other entry has a value of 1 or more, where the chain's round-off
# (a few 2^-53 relative) is orders below the float32 ulp.
EXACT_IDENTITIES = [(64, 64, 0.5), (64, 32, 0.5), (32, 64, 1.0), (128, 64, 2.0)]


@pytest.mark.parametrize("width,height,focal", EXACT_IDENTITIES)
def test_identity_mapping_is_the_pixel_grid_exactly(emu, width, height, focal):
    """a perspective camera with k1 = k2 = 0 mapped to perspective_camera_from_perspective of itself: map1[v, u] == u and
    map2[v, u] == v in every entry, and the undistorted image equals the input byte for byte"""
    from opensfm_amd import undistort

    cam, new = identity_pair(undistort, width, height, focal)
    map1, map2 = undistort.compute_camera_mapping(cam, new, width, height)
    v, u = np.indices((height, width))
    print(f"map1: {int((map1 != u).sum())} entries differ, largest {float(np.abs(map1 - u).max())}; "
          f"map2: {int((map2 != v).sum())} entries differ, largest {float(np.abs(map2 - v).max())}")
    assert np.array_equal(map1, u.astype(np.float32)) and np.array_equal(map2, v.astype(np.float32))
    assert not np.signbit(map1).any() and not np.signbit(map2).any()  # +0, not -0
    want = cases.camera_mapping(("perspective", [0.0, 0.0, focal]), ("perspective", [0.0, 0.0, focal]), width, height)
    assert np.array_equal(want[0], map1) and np.array_equal(want[1], map2)
    image = np.random.default_rng(3).integers(0, 256, (height, width, 3), dtype=np.uint8)
    for interpolation in (undistort.INTER_AREA, undistort.INTER_NEAREST):
        out, _ = undistort.undistort_raw([image], [0], [cam], [new], interpolation)
        assert np.array_equal(out[0], image)


def test_identity_at_a_general_size_is_the_grid_wherever_the_value_is_not_zero(emu):
    """37 x 29, focal 0.8: none of the scalings is exact.  Entries of value 1 or more equal the grid; an entry of value 0 may keep the
    residue of cancelling -half against +half in the literal double chain (measured: 2 of 1073 entries of map2, row 0, -1.78e-15) --
    the plain restatement of ComputeCameraMapping's text has the same bits there, so the reference leaves them too.  They are far
    inside the 1/64 of a pixel the fixed-point split rounds away: the image comes back byte for byte."""
    from opensfm_amd import undistort

    cam, new = identity_pair(undistort)
    got = undistort.compute_camera_mapping(cam, new, 37, 29)
    want = cases.camera_mapping(("perspective", [0.0, 0.0, 0.8]), ("perspective", [0.0, 0.0, 0.8]), 37, 29)
    assert all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want))
    v, u = np.indices((29, 37))
    assert np.array_equal(got[0][:, 1:], u[:, 1:].astype(np.float32)) and np.array_equal(got[1][1:], v[1:].astype(np.float32))
    half_ulp = 14.5 * 2.0 ** -52  # one double ulp of the larger half-size
    assert np.abs(got[0][:, 0]).max() <= 4 * half_ulp and np.abs(got[1][0]).max() <= 4 * half_ulp
    image = np.random.default_rng(3).integers(0, 256, (29, 37, 3), dtype=np.uint8)
    for interpolation in (undistort.INTER_AREA, undistort.INTER_NEAREST):
        out, _ = undistort.undistort_raw([image], [0], [cam], [new], interpolation)
        assert np.array_equal(out[0], image)


# ---- 5. an independent bound on linear interpolation ----
@pytest.mark.parametrize("kind", ["random", "smooth"])
def test_linear_interpolation_is_within_the_bound_of_the_exact_bilinear_value(emu, kind):
    """|out - exact| <= 0.5 + range / 32: the coordinates are off by at most 1/64 per axis, each moving the value by at most range / 64,
    and the final rounding adds at most 0.5"""
    from opensfm_amd import undistort

    rng = np.random.default_rng(17)
    w, h = 41, 23
    if kind == "random":
        src = rng.integers(0, 256, (h, w), dtype=np.uint8)
    else:
        yy, xx = np.indices((h, w))
        src = np.clip(np.round(120 + 60 * np.sin(xx / 7.0) + 50 * np.cos(yy / 5.0)), 0, 255).astype(np.uint8)
    map1 = rng.uniform(-1.5, w + 0.5, (31, 45)).astype(np.float32)
    map2 = rng.uniform(-1.5, h + 0.5, (31, 45)).astype(np.float32)
    for got in (undistort.remap(src, map1, map2, undistort.INTER_LINEAR), cases.remap(src, map1, map2, cases.INTER_LINEAR)):
        worst = 0.0
        for v in range(map1.shape[0]):
            for u in range(map1.shape[1]):
                exact, spread = cases.exact_bilinear(src, map1[v, u], map2[v, u])
                worst = max(worst, abs(float(got[v, u]) - float(exact)) - (0.5 + float(spread) / 32))
        print(f"{kind}: largest |out - exact| - bound = {worst}")
        assert worst <= 1e-9


# ---- 6. scaled output ----
@pytest.mark.parametrize("max_size", [20, 36, 37, 64, 100])
def test_scaled_output_equals_full_remap_then_nearest_resize(emu, max_size):
    from opensfm_amd import undistort

    src, map1, map2 = cases.remap_case("37x29")
    h, w = undistort.scale_image_size(29, 37, max_size)
    assert (h, w) == cases.scale_size(29, 37, max_size) and ((h, w) == (29, 37)) == (max_size >= 37)
    for interpolation in (cases.INTER_LINEAR, cases.INTER_NEAREST):
        want = cases.scale_image(cases.remap(src, map1, map2, interpolation), max_size)
        got = undistort.remap(src, map1, map2, interpolation, out_size=(h, w))
        assert got.shape == want.shape and np.array_equal(got, want)
    # the fused path scales the same way
    (fm, fp), (tm, tp) = cases.MAPPING_CASES["brown"]
    image = np.random.default_rng(5).integers(0, 256, (29, 37, 3), dtype=np.uint8)
    m = cases.load("mapping_37x29")
    want = cases.scale_image(cases.remap(image, m["brown_map1"], m["brown_map2"], cases.INTER_LINEAR), max_size)
    got, _ = undistort.undistort_raw([image], [0], [camera(fm, fp)], [camera(tm, tp)], undistort.INTER_AREA, [(h, w)])
    assert np.array_equal(got[0], want)


def test_python_round_decides_the_scaled_size():
    from opensfm_amd import undistort

    assert undistort.scale_image_size(3, 5, 2) == (1, 2) == cases.scale_size(3, 5, 2)  # 1.2 -> 1, 2.0 -> 2
    assert undistort.scale_image_size(5, 20, 10) == (2, 10)  # 2.5 rounds half to even
    assert undistort.scale_image_size(48, 64, 64) == (48, 64) and undistort.scale_image_size(48, 64, 1000) == (48, 64)


# ---- 7. the fused path and batches on the emulation ----
def test_fused_undistortion_equals_mapping_then_remap_and_batches_equal_single_calls(emu):
    from opensfm_amd import undistort

    rng = np.random.default_rng(9)
    shapes = [(29, 37, 3), (33, 65), (48, 64, 4), (29, 37)]
    images = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    froms = [camera(*cases.MAPPING_CASES[n][0]) for n in ("brown", "fisheye")]
    tos = [camera(*cases.MAPPING_CASES[n][1]) for n in ("brown", "fisheye")]
    cam_of = [0, 1, 0, 1]
    for interpolation in (undistort.INTER_AREA, undistort.INTER_NEAREST):
        together, _ = undistort.undistort_raw(images, cam_of, froms, tos, interpolation)
        again, _ = undistort.undistort_raw(images, cam_of, froms, tos, interpolation)
        for k, image in enumerate(images):
            alone, _ = undistort.undistort_raw([image], [0], [froms[cam_of[k]]], [tos[cam_of[k]]], interpolation)
            map1, map2 = undistort.compute_camera_mapping(froms[cam_of[k]], tos[cam_of[k]], image.shape[1], image.shape[0])
            assert np.array_equal(together[k], alone[0]) and np.array_equal(together[k], again[k])
            assert np.array_equal(together[k], undistort.remap(image, map1, map2, interpolation))
            assert np.array_equal(together[k], cases.remap(image, map1, map2, interpolation))  # the restatement on the library's map
        assert (together[0] == 0).all(axis=2).any() and together[0].any()  # corners read outside the source
    m1, m2 = undistort.compute_camera_mapping(froms[0], tos[0], 37, 29)
    other = np.ascontiguousarray(m2[::-1])  # two entries that share map1 but not map2 keep their own map2
    pair, _ = undistort.remap_raw([images[0], images[0]], [(m1, m2), (m1, other)], undistort.INTER_LINEAR)
    assert np.array_equal(pair[0], cases.remap(images[0], m1, m2, cases.INTER_LINEAR))
    assert np.array_equal(pair[1], cases.remap(images[0], m1, other, cases.INTER_LINEAR)) and not np.array_equal(pair[0], pair[1])
    assert undistort.undistort_raw([], [], froms, tos, undistort.INTER_AREA)[0] == []
    assert undistort.remap_raw([], [], undistort.INTER_LINEAR)[0] == []
    assert undistort.compute_camera_mappings([])[0] == []


# ---- 8. the stand-alone program under ASan + UBSan ----
@pytest.mark.parametrize("name,mode,model", [("37x29", "linear_wrap", "brown"), ("65x33x3", "linear_constant", "fisheye"),
                                             ("130x70x4", "nearest_constant", "perspective"), ("1x1", "nearest_wrap", "radial")])
def test_standalone_program_under_sanitizers(tmp_path, name, mode, model):
    exe = _builder().build_main("undistort_main")
    src, map1, map2 = cases.remap_case(name)
    interpolation, border = cases.MODES[mode]
    h, w = src.shape[:2]
    c = 1 if src.ndim == 2 else src.shape[2]
    out_h, out_w = cases.scale_size(h, w, max(1, (2 * max(h, w)) // 3))
    (fm, fp), (tm, tp) = cases.MAPPING_CASES[model]
    head = np.array([w, h, c, map1.shape[1], map1.shape[0], out_w, out_h, interpolation, border, cases.MODEL_IDS[fm], cases.MODEL_IDS[tm], 0], np.int32)
    problem, result = tmp_path / "problem.bin", tmp_path / "result.bin"
    problem.write_bytes(head.tobytes() + cases.pad16(fp).tobytes() + cases.pad16(tp).tobytes() + src.tobytes() + map1.tobytes() + map2.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(problem), str(result)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    data = result.read_bytes()
    at = 0

    def take(count, dtype, shape):
        nonlocal at
        a = np.frombuffer(data, dtype, count, at).reshape(shape)
        at += a.nbytes
        return a

    tail = () if c == 1 else (c,)
    remapped = take(map1.size * c, np.uint8, map1.shape + tail)
    cam1, cam2 = take(w * h, np.float32, (h, w)), take(w * h, np.float32, (h, w))
    fused = take(out_w * out_h * c, np.uint8, (out_h, out_w) + tail)
    first, second = take(fused.size, np.uint8, fused.shape), take(fused.size, np.uint8, fused.shape)
    assert at == len(data)
    assert np.array_equal(remapped, cases.load("remap_" + name)[mode])
    want1, want2 = cases.camera_mapping((fm, fp), (tm, tp), w, h)
    check_mapping(model, (cam1, cam2), (want1, want2))
    want = cases.resize_nearest(cases.remap(src, cam1, cam2, interpolation), out_w, out_h)
    assert np.array_equal(fused, want) and np.array_equal(first, want) and np.array_equal(second, want)


# ---- 9. the Python mirror of opensfm/undistort.py ----
def test_focal_rules_of_the_camera_constructors():
    from opensfm_amd import undistort
    from opensfm_amd.geometry_types import Camera

    def dressed(c):
        c.id, c.width, c.height = "cam", 640, 480
        return c

    wide = dict(focal=0.6, aspect_ratio=1.1, principal_point=[0.01, -0.02])
    cams = {"perspective": dressed(Camera.create_perspective(0.7, 0.1, 0.01)), "fisheye": dressed(Camera.create_fisheye(0.7, 0.1, 0.01)),
            "brown": dressed(Camera.create_brown(distortion=[0.1, 0.01, 0.001, 0.002, 0.003], **wide)),
            "fisheye_opencv": dressed(Camera.create_fisheye_opencv(distortion=[0.1, 0.01, 0.001, 0.002], **wide)),
            "fisheye62": dressed(Camera.create_fisheye62(distortion=[0.1] * 8, **wide))}
    rules = {"perspective": (undistort.perspective_camera_from_perspective, 0.7), "fisheye": (undistort.perspective_camera_from_fisheye, 0.7),
             "brown": (undistort.perspective_camera_from_brown, 0.6 * (1 + 1.1) / 2.0),
             "fisheye_opencv": (undistort.perspective_camera_from_fisheye_opencv, 0.6 * (1 + 1.1) / 2.0),
             "fisheye62": (undistort.perspective_camera_from_fisheye62, 0.6 * (1 + 1.1) / 2.0)}
    for kind, (make, focal) in rules.items():
        for new in (make(cams[kind]), undistort.undistorted_camera(cams[kind])):
            assert new.projection_type == "perspective" and new.focal == focal and new.k1 == 0.0 and new.k2 == 0.0
            assert (new.id, new.width, new.height) == ("cam", 640, 480)
        assert cases.undistorted_focal(kind, list(_native(cams[kind]))) == focal
    for kind in ("fisheye624", "dual", "radial", "simple_radial", "spherical"):
        with pytest.raises(NotImplementedError, match="Undistort not implemented for projection type: " + kind):
            undistort.undistorted_camera(Camera(kind))


def _native(cam):
    from opensfm_amd.geometry_types import camera_parameter_values

    return camera_parameter_values(cam)[: {"perspective": 3, "fisheye": 3, "brown": 9, "fisheye_opencv": 8, "fisheye62": 12}[cam.projection_type]]


def panorama_scene(undistort):
    from opensfm_amd.geometry_types import Camera, Pose, Reconstruction

    rec, urec = Reconstruction(), Reconstruction()
    pano_cam = Camera.create_spherical()
    pano_cam.id, pano_cam.width, pano_cam.height = "pano", 2048, 1024
    rec.add_camera(pano_cam)
    pose = Pose()
    pose.set_rotation_matrix(cases.panorama_pose_rotation())
    pose.translation = np.array([1.0, -2.0, 0.5])
    shot = rec.create_shot("pano.jpg", "pano", pose)
    views = undistort.perspective_views_of_a_panorama(shot, cases.PANORAMA["view"], urec, "jpg", itertools.count(3))
    return shot, views, urec


def test_six_panorama_views_have_the_references_names_and_rotations():
    from opensfm_amd import undistort

    shot, views, urec = panorama_scene(undistort)
    assert [v.id for v in views] == [f"pano.jpg_perspective_view_{n}.jpg" for n in cases.VIEW_NAMES]
    assert undistort.PANORAMA_VIEW_NAMES == ["front", "left", "back", "right", "top", "bottom"]
    assert list(urec.rig_instances) == ["3"] and sorted(urec.rig_cameras) == sorted(cases.VIEW_NAMES)
    cam = urec.cameras["perspective_panorama_camera"]
    assert (cam.projection_type, cam.focal, cam.k1, cam.k2, cam.width, cam.height) == ("perspective", 0.5, 0.0, 0.0, 32, 32)
    R_pano = shot.pose.get_rotation_matrix()
    y, x = np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0])
    for view, R_view, (axis, angle) in zip(views, cases.view_rotations(), [(y, 0.0), (y, -np.pi / 2), (y, -np.pi), (y, -3 * np.pi / 2),
                                                                           (x, -np.pi / 2), (x, np.pi / 2)]):
        assert view.camera is cam and view.metadata is shot.metadata
        assert np.abs(view.rig_camera.pose.get_rotation_matrix() - R_view).max() < 1e-12
        assert np.abs(view.pose.get_rotation_matrix() - R_view @ R_pano).max() < 1e-12  # rig camera o rig instance
        assert np.abs(R_view @ axis - axis).max() < 1e-12  # about that axis ...
        assert abs(np.trace(R_view) - (1 + 2 * np.cos(angle))) < 1e-12  # ... by that angle
    assert np.abs(views[1].rig_camera.pose.get_rotation_matrix() @ np.array([0, 0, 1.0]) - np.array([-1.0, 0, 0])).max() < 1e-12
    assert np.abs(views[0].pose.translation - shot.pose.translation).max() < 1e-12


def test_panorama_views_on_the_emulation(emu):
    from opensfm_amd import undistort

    shot, views, _ = panorama_scene(undistort)
    image = cases.panorama_image()
    maps, _ = undistort.panorama_mappings(shot.camera, [(v.camera, undistort._view_rotation(shot, v)) for v in views], 128, 64)
    # (the rotations here come from poses, an angle-axis round trip away from the matrices of the stored maps: the next test pins the
    # maps, this one the map-then-remap scheme on the library's own maps)
    for interpolation, label in ((undistort.INTER_AREA, "linear"), (undistort.INTER_NEAREST, "nearest")):
        got = undistort.undistort_image(shot, views, image, interpolation, 1000)
        assert list(got) == [v.id for v in views]
        for v, (x, y) in zip(views, maps):
            assert np.array_equal(got[v.id], cases.remap(image, x, y, cases.MODES[label + "_wrap"][0], cases.BORDER_WRAP))
    with pytest.raises(ValueError, match="128 x 64"):
        undistort.undistort_image(shot, views, image[:, :100], undistort.INTER_AREA, 1000)


def test_panorama_mapping_with_the_stored_rotations_equals_the_restatement(emu):
    from opensfm_amd import undistort

    stored, R_pano = cases.load("panorama"), cases.panorama_pose_rotation()
    view_cam = camera("perspective", [0.0, 0.0, 0.5])
    view_cam.width = view_cam.height = 32
    maps, _ = undistort.panorama_mappings(camera("spherical", []), [(view_cam, np.dot(R_pano, R.T)) for R in cases.view_rotations()], 128, 64)
    seam = 0
    for name, (x, y) in zip(cases.VIEW_NAMES, maps):
        worst = max(int(cases.ulp_distance(x, stored[name + "_x"]).max()), int(cases.ulp_distance(y, stored[name + "_y"]).max()))
        print(f"{name}: {worst} float32 ulp")
        assert worst <= 1, (name, worst)
        seam += bool((x < 1).any() and (x > 126).any())
    assert seam >= 1  # a view straddles the +-pi seam


def test_undistort_image_and_undistort_images_as_the_reference_calls_them(emu):
    from opensfm_amd import undistort
    from opensfm_amd.geometry_types import Reconstruction

    rng = np.random.default_rng(23)
    rec, urec = Reconstruction(), Reconstruction()
    cams = {"a": camera(*cases.MAPPING_CASES["brown"][0]), "b": camera(*cases.MAPPING_CASES["fisheye"][0])}
    for cid, c in cams.items():
        c.id, c.width, c.height = cid, 64, 48
        rec.add_camera(c)
        urec.add_camera(undistort.undistorted_camera(c))
    shots = [rec.create_shot(f"im{k}", cid) for k, cid in enumerate("aba")]
    ushots = [urec.create_shot(undistort.add_image_format_extension(s.id, "jpg"), s.camera.id, s.pose) for s in shots]
    images = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8) for _ in shots]
    masks = [rng.integers(0, 2, (48, 64), dtype=np.uint8) * 255, None, rng.integers(0, 2, (48, 64), dtype=np.uint8)]
    segmentations = [None, rng.integers(0, 20, (48, 64), dtype=np.uint8), None]
    max_size = 40
    batch = undistort.undistort_images(shots, images, masks, segmentations, max_size)
    for k, shot in enumerate(shots):
        fm, fp = shot.camera.projection_type, list(_native(shot.camera))
        m = cases.camera_mapping((fm, fp), ("perspective", [0.0, 0.0, cases.undistorted_focal(fm, fp)]), 64, 48)
        lib_map = undistort.compute_camera_mapping(shot.camera, ushots[k].camera, 64, 48)
        assert max(int(cases.ulp_distance(a, b).max()) for a, b in zip(lib_map, m)) <= (0 if fm == "brown" else 1)
        for kind, arrays, interpolation in (("image", images, undistort.INTER_AREA), ("mask", masks, undistort.INTER_NEAREST),
                                            ("segmentation", segmentations, undistort.INTER_NEAREST)):
            one = undistort.undistort_image(shot, [ushots[k]], arrays[k], interpolation, max_size)
            if arrays[k] is None:
                assert one == {} and batch[k][kind] is None
                continue
            want = cases.scale_image(cases.remap(arrays[k], lib_map[0], lib_map[1], interpolation), max_size)
            assert list(one) == [f"im{k}.jpg"] and want.shape[:2] == (30, 40)
            assert np.array_equal(one[f"im{k}.jpg"], want) and np.array_equal(batch[k][kind], want)


# ---- 10. refusals ----
def test_refusals(emu):
    from opensfm_amd import _lib, undistort

    cam, new = camera(*cases.MAPPING_CASES["brown"][0]), camera(*cases.MAPPING_CASES["brown"][1])
    image = np.full((6, 8, 3), 9, np.uint8)
    map1, map2 = np.zeros((6, 8), np.float32), np.zeros((6, 8), np.float32)

    def refused(call, needle):
        with pytest.raises(_lib.OsfmError, match=r"\(-1\)") as e:
            call()
        assert needle in str(e.value), str(e.value)

    refused(lambda: undistort.remap(np.zeros((6, 8, 2), np.uint8), map1, map2, undistort.INTER_LINEAR), "2 channels")
    refused(lambda: undistort.remap(image.astype(np.uint16), map1, map2, undistort.INTER_LINEAR), "uint16")
    refused(lambda: undistort.undistort_raw([image.astype(np.uint16)], [0], [cam], [new], undistort.INTER_AREA), "uint16")
    refused(lambda: undistort.remap(np.zeros((0, 8), np.uint8), map1, map2, undistort.INTER_LINEAR), "not positive")
    refused(lambda: undistort.remap(image, map1, map2, undistort.INTER_LINEAR, out_size=(6, 32768)), "32767")
    refused(lambda: undistort.compute_camera_mapping(cam, new, 32768, 4), "32767")
    refused(lambda: undistort.compute_camera_mapping(cam, new, 0, 4), "not positive")
    refused(lambda: undistort.undistort_raw([image], [1], [cam], [new], undistort.INTER_AREA), "outside the table")
    refused(lambda: undistort.undistort_raw([image], [-1], [cam], [new], undistort.INTER_AREA), "outside the table")
    for bad in (float("nan"), float("inf")):
        broken = camera(*cases.MAPPING_CASES["brown"][0])
        broken.k2 = bad
        refused(lambda: undistort.compute_camera_mapping(broken, new, 8, 6), "not finite")
        refused(lambda: undistort.undistort_raw([image], [0], [broken], [new], undistort.INTER_AREA), "not finite")
    view = camera("perspective", [0.0, 0.0, 0.5])
    view.width = view.height = 8
    for bad in (float("nan"), float("-inf")):
        rotation = np.eye(3)
        rotation[1, 2] = bad
        refused(lambda: undistort.panorama_mappings(camera("spherical", []), [(view, rotation)], 32, 16), "rotation is not finite")
    with pytest.raises(ValueError):
        undistort.remap(image, map1, map2, 2)  # cv2.INTER_CUBIC
    with pytest.raises(ValueError):
        undistort.remap(image, map1, map2, undistort.INTER_LINEAR, border="reflect")
    # the C ABI itself refuses unknown interpolation and border values, and a refused call leaves the output alone
    lib, ctx = _lib.load(), _lib.default_context()
    out = np.full((6, 8, 3), 0xA5, np.uint8)
    w, h, c = np.array([8], np.int32), np.array([6], np.int32), np.array([3], np.int32)
    ip, vp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: (C.c_void_p * 1)(a.ctypes.data))
    for interpolation, border in ((2, 0), (1, 1), (-1, 0), (1, 4)):
        rc = lib.osfm_remap_images(ctx.handle, 1, vp(image), ip(w), ip(h), ip(c), vp(map1), vp(map2), ip(w), ip(h), ip(w), ip(h), interpolation,
                                   border, vp(out), None)
        assert rc == -1 and (out == 0xA5).all() and b"unknown" in lib.osfm_last_error()
    # ... kernel_ms included: it is written by calls that succeed
    ms = C.c_double(-7.0)
    assert lib.osfm_remap_images(ctx.handle, 1, vp(image), ip(w), ip(h), ip(c), vp(map1), vp(map2), ip(w), ip(h), ip(w), ip(h), 2, 0, vp(out),
                                 C.byref(ms)) == -1 and ms.value == -7.0
    assert lib.osfm_remap_images(ctx.handle, 1, vp(image), ip(w), ip(h), ip(c), vp(map1), vp(map2), ip(w), ip(h), ip(w), ip(h), 1, 0, vp(out),
                                 C.byref(ms)) == 0 and ms.value >= 0.0 and (out == 9).all()
    with pytest.raises(NotImplementedError, match="Undistort not implemented for projection type: dual"):
        undistort.undistort_image(type("S", (), {"camera": camera("dual", [0.5, 0.0, 0.0, 0.6]), "id": "x"})(), [], image, undistort.INTER_AREA, 100)
