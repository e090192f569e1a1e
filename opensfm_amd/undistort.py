"""Image undistortion on the GPU: ``opensfm/undistort.py`` over the camera and shot objects of ``geometry_types`` (attributes as in the
reference).  ``pygeometry.compute_camera_mapping`` is ``osfm_camera_mapping``, ``cv2.remap`` is ``osfm_remap_images``, ``undistort_image``
for a frame camera is the fused ``osfm_undistort_images`` (no map is stored), and ``scale_image``'s nearest resize is folded into the
remap: only the pixels that survive it are computed.  There is no CPU fallback.

cv2.remap and cv2.resize are restated, not compared with OpenCV (``include/osfm_mi355.h`` states the rules and the divergences).  Out of
scope: cv2's ``INTER_AREA`` *resize* of a panorama to ``4 w x 2 w`` -- ``undistort_image`` takes a panorama that already has that size
and raises ``ValueError`` otherwise; uint16 images are refused, not converted."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .geometry_types import Camera, Pose, RigCamera, RigInstance
from .matching import camera_parameters

INTER_NEAREST, INTER_LINEAR, INTER_AREA = 0, 1, 3  # cv2's values (OSFM_INTER_*)
BORDER_CONSTANT, BORDER_WRAP = 0, 3                # cv2's values (OSFM_BORDER_*)
_BORDERS = {"constant": BORDER_CONSTANT, "wrap": BORDER_WRAP, BORDER_CONSTANT: BORDER_CONSTANT, BORDER_WRAP: BORDER_WRAP}
FRAME_PROJECTIONS = ("perspective", "brown", "fisheye", "fisheye_opencv", "fisheye62")
PANORAMA_PROJECTIONS = ("spherical", "equirectangular")  # pygeometry.Camera.is_panorama
OSFM_E_INVALID = -1


# ---- the undistorted cameras (undistort.py:253-307) ----
def _perspective(distorted, focal: float) -> Camera:
    camera = Camera.create_perspective(focal, 0.0, 0.0)
    camera.id = distorted.id
    camera.width = distorted.width
    camera.height = distorted.height
    return camera


def perspective_camera_from_perspective(distorted) -> Camera:
    """Create an undistorted camera from a distorted."""
    return _perspective(distorted, distorted.focal)


def perspective_camera_from_brown(brown) -> Camera:
    """Create a perspective camera from a Brown camera."""
    return _perspective(brown, brown.focal * (1 + brown.aspect_ratio) / 2.0)


def perspective_camera_from_fisheye(fisheye) -> Camera:
    """Create a perspective camera from a fisheye."""
    return _perspective(fisheye, fisheye.focal)


def perspective_camera_from_fisheye_opencv(fisheye_opencv) -> Camera:
    """Create a perspective camera from a fisheye extended."""
    return _perspective(fisheye_opencv, fisheye_opencv.focal * (1 + fisheye_opencv.aspect_ratio) / 2.0)


def perspective_camera_from_fisheye62(fisheye62) -> Camera:
    """Create a perspective camera from a fisheye extended."""
    return _perspective(fisheye62, fisheye62.focal * (1 + fisheye62.aspect_ratio) / 2.0)


_UNDISTORTED = {"perspective": perspective_camera_from_perspective, "brown": perspective_camera_from_brown,
                "fisheye": perspective_camera_from_fisheye, "fisheye_opencv": perspective_camera_from_fisheye_opencv,
                "fisheye62": perspective_camera_from_fisheye62}


def undistorted_camera(camera) -> Camera:
    """the perspective camera ``undistort_reconstruction`` pairs with a frame camera"""
    if camera.projection_type not in _UNDISTORTED:
        raise NotImplementedError("Undistort not implemented for projection type: {}".format(camera.projection_type))
    return _UNDISTORTED[camera.projection_type](camera)


# ---- plumbing ----
def _pointers(arrays: Sequence[np.ndarray]):
    return (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])


def _i32(values) -> np.ndarray:
    return np.ascontiguousarray(values, np.int32).reshape(-1)


def _ip(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _camera_table(cameras) -> Tuple[np.ndarray, np.ndarray]:
    pairs = [camera_parameters(c) for c in cameras]
    models = _i32([m for m, _ in pairs])
    params = np.ascontiguousarray(np.concatenate([p for _, p in pairs]) if pairs else np.zeros(0), np.float64)
    return models, params


def _image(image) -> np.ndarray:
    """a contiguous (h, w) or (h, w, c) uint8 array; any other dtype is refused (uint16 is what ``anydepth`` loads)"""
    a = np.asarray(image)
    if a.dtype != np.uint8:
        raise _lib.OsfmError(f"undistort failed ({OSFM_E_INVALID}): images must be uint8, not {a.dtype} (not converted silently)")
    if a.ndim not in (2, 3):
        raise _lib.OsfmError(f"undistort failed ({OSFM_E_INVALID}): an image must be (height, width) or (height, width, channels)")
    return np.ascontiguousarray(a)


def _channels(a: np.ndarray) -> int:
    return 1 if a.ndim == 2 else a.shape[2]


def _out_array(a: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    return np.zeros((out_h, out_w) + a.shape[2:], np.uint8)


def _interpolation(interpolation: int) -> int:
    if interpolation not in (INTER_NEAREST, INTER_LINEAR, INTER_AREA):
        raise ValueError(f"interpolation must be INTER_NEAREST, INTER_LINEAR or INTER_AREA, not {interpolation!r}")
    return int(interpolation)


def scale_image_size(h: int, w: int, max_size: int) -> Tuple[int, int]:
    """(height, width) of ``scale_image(image, max_size)`` for an image of (h, w): unchanged when it fits"""
    factor = max_size / float(max(h, w))
    if factor >= 1:
        return h, w
    return int(round(h * factor)), int(round(w * factor))


# ---- the calls ----
def compute_camera_mappings(pairs: Sequence[tuple], device: Optional[int] = None) -> Tuple[List[Tuple[np.ndarray, np.ndarray]], float]:
    """``osfm_camera_mapping`` for a list of (from_camera, to_camera, width, height): [(map1, map2)], kernel ms"""
    fm, fp = _camera_table([p[0] for p in pairs])
    tm, tp = _camera_table([p[1] for p in pairs])
    widths, heights = _i32([p[2] for p in pairs]), _i32([p[3] for p in pairs])
    maps = [(np.zeros((max(int(p[3]), 0), max(int(p[2]), 0)), np.float32), np.zeros((max(int(p[3]), 0), max(int(p[2]), 0)), np.float32)) for p in pairs]
    ms = C.c_double(0.0)
    ctx = _lib.default_context(device)
    _lib.check(_lib.load().osfm_camera_mapping(ctx.handle, len(pairs), _ip(fm), _dp(fp), _ip(tm), _dp(tp), _ip(widths), _ip(heights),
                                               _pointers([m[0] for m in maps]), _pointers([m[1] for m in maps]), C.byref(ms)),
               "osfm_camera_mapping")
    return maps, ms.value


def compute_camera_mapping(from_camera, to_camera, width: int, height: int) -> Tuple[np.ndarray, np.ndarray]:
    """``pygeometry.compute_camera_mapping``: (map1, map2), float32 of shape (height, width)"""
    return compute_camera_mappings([(from_camera, to_camera, width, height)])[0][0]


def panorama_mappings(pano_camera, views: Sequence[tuple], pano_width: int, pano_height: int,
                      device: Optional[int] = None) -> Tuple[List[Tuple[np.ndarray, np.ndarray]], float]:
    """``osfm_panorama_mapping``: the float32 maps ``render_perspective_view_of_a_panorama`` hands to cv2.remap, for a list of
    (view_camera, rotation) with rotation = R_pano R_view^T (3 x 3): [(x, y)], kernel ms"""
    fm, fp = _camera_table([pano_camera] * len(views))
    tm, tp = _camera_table([v[0] for v in views])
    rotations = np.ascontiguousarray(np.concatenate([np.asarray(v[1], np.float64).reshape(9) for v in views]) if views else np.zeros(0))
    widths, heights = _i32([v[0].width for v in views]), _i32([v[0].height for v in views])
    src_w, src_h = _i32([pano_width] * len(views)), _i32([pano_height] * len(views))
    maps = [(np.zeros((max(int(h), 0), max(int(w), 0)), np.float32), np.zeros((max(int(h), 0), max(int(w), 0)), np.float32))
            for w, h in zip(widths, heights)]
    ms = C.c_double(0.0)
    ctx = _lib.default_context(device)
    _lib.check(_lib.load().osfm_panorama_mapping(ctx.handle, len(views), _ip(fm), _dp(fp), _ip(tm), _dp(tp), _dp(rotations), _ip(src_w), _ip(src_h),
                                                 _ip(widths), _ip(heights), _pointers([m[0] for m in maps]), _pointers([m[1] for m in maps]),
                                                 C.byref(ms)), "osfm_panorama_mapping")
    return maps, ms.value


def remap_raw(images: Sequence[np.ndarray], maps: Sequence[Tuple[np.ndarray, np.ndarray]], interpolation: int, border=BORDER_CONSTANT,
              out_sizes: Optional[Sequence[Optional[Tuple[int, int]]]] = None, device: Optional[int] = None) -> Tuple[List[np.ndarray], float]:
    """``osfm_remap_images``: image i through maps[i] (entries may be the same arrays: uploaded once); out_sizes[i] = (height, width) of a
    nearest-resized result or None: [remapped], kernel ms"""
    if border not in _BORDERS:
        raise ValueError(f"border must be 'constant' or 'wrap', not {border!r}")
    images = [_image(im) for im in images]
    if len(maps) != len(images):
        raise ValueError("one (map1, map2) per image")
    checked = {}
    for m1, m2 in maps:  # (shared maps are converted once and keep one address)
        if (id(m1), id(m2)) not in checked:
            a, b = np.ascontiguousarray(m1, np.float32), np.ascontiguousarray(m2, np.float32)
            if a.ndim != 2 or a.shape != b.shape:
                raise ValueError("map1 and map2 must be (height, width) arrays of one shape")
            checked[(id(m1), id(m2))] = (a, b)
    maps = [checked[(id(m1), id(m2))] for m1, m2 in maps]
    sizes = [(m[0].shape if out_sizes is None or out_sizes[i] is None else tuple(int(v) for v in out_sizes[i])) for i, m in enumerate(maps)]
    outs = [_out_array(im, size[1], size[0]) for im, size in zip(images, sizes)]
    ms = C.c_double(0.0)
    ctx = _lib.default_context(device)
    _lib.check(_lib.load().osfm_remap_images(
        ctx.handle, len(images), _pointers(images), _ip(_i32([im.shape[1] for im in images])), _ip(_i32([im.shape[0] for im in images])),
        _ip(_i32([_channels(im) for im in images])), _pointers([m[0] for m in maps]), _pointers([m[1] for m in maps]),
        _ip(_i32([m[0].shape[1] for m in maps])), _ip(_i32([m[0].shape[0] for m in maps])), _ip(_i32([s[1] for s in sizes])),
        _ip(_i32([s[0] for s in sizes])), _interpolation(interpolation), _BORDERS[border], _pointers(outs), C.byref(ms)), "osfm_remap_images")
    return outs, ms.value


def remap(images, map1: np.ndarray, map2: np.ndarray, interpolation: int, border="constant", out_size: Optional[Tuple[int, int]] = None):
    """``cv2.remap(image, map1, map2, interpolation, borderMode=border)`` for one image or a list of images that share the map;
    out_size = (height, width): followed by ``cv2.resize(..., INTER_NEAREST)`` to that size (only the surviving pixels are computed)"""
    single = isinstance(images, np.ndarray)
    batch = [images] if single else list(images)
    outs, _ = remap_raw(batch, [(map1, map2)] * len(batch), interpolation, border, [out_size] * len(batch))
    return outs[0] if single else outs


def undistort_raw(images: Sequence[np.ndarray], image_cam: Sequence[int], from_cameras: Sequence, to_cameras: Sequence, interpolation: int,
                  out_sizes: Optional[Sequence[Optional[Tuple[int, int]]]] = None, device: Optional[int] = None) -> Tuple[List[np.ndarray], float]:
    """``osfm_undistort_images``: image i through the camera pair image_cam[i] of (from_cameras, to_cameras): [undistorted], kernel ms"""
    images = [_image(im) for im in images]
    fm, fp = _camera_table(from_cameras)
    tm, tp = _camera_table(to_cameras)
    sizes = [(im.shape[:2] if out_sizes is None or out_sizes[i] is None else tuple(int(v) for v in out_sizes[i])) for i, im in enumerate(images)]
    outs = [_out_array(im, size[1], size[0]) for im, size in zip(images, sizes)]
    ms = C.c_double(0.0)
    ctx = _lib.default_context(device)
    _lib.check(_lib.load().osfm_undistort_images(
        ctx.handle, len(images), _pointers(images), _ip(_i32([im.shape[1] for im in images])), _ip(_i32([im.shape[0] for im in images])),
        _ip(_i32([_channels(im) for im in images])), _ip(_i32(list(image_cam))), len(fm), _ip(fm), _dp(fp), _ip(tm), _dp(tp),
        _ip(_i32([s[1] for s in sizes])), _ip(_i32([s[0] for s in sizes])), _interpolation(interpolation), _pointers(outs), C.byref(ms)),
        "osfm_undistort_images")
    return outs, ms.value


# ---- opensfm/undistort.py ----
def add_image_format_extension(shot_id: str, image_format: str) -> str:
    return shot_id if shot_id.endswith(f".{image_format}") else f"{shot_id}.{image_format}"


def _axis_rotation(angle: float, axis) -> np.ndarray:
    """``transformations.rotation_matrix(angle, axis)[:3, :3]`` (opensfm/transformations.py)"""
    sina, cosa = np.sin(angle), np.cos(angle)
    d = np.asarray(axis, float)
    d = d / np.sqrt(np.dot(d, d))
    R = np.diag([cosa, cosa, cosa])
    R += np.outer(d, d) * (1.0 - cosa)
    d = d * sina
    R += np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
    return R


PANORAMA_VIEW_NAMES = ["front", "left", "back", "right", "top", "bottom"]


def panorama_view_rotations() -> List[np.ndarray]:
    """the rig camera rotations of the six views (undistort.py:325-332)"""
    return [_axis_rotation(-0 * np.pi / 2, [0, 1, 0]), _axis_rotation(-1 * np.pi / 2, [0, 1, 0]), _axis_rotation(-2 * np.pi / 2, [0, 1, 0]),
            _axis_rotation(-3 * np.pi / 2, [0, 1, 0]), _axis_rotation(-np.pi / 2, [1, 0, 0]), _axis_rotation(+np.pi / 2, [1, 0, 0])]


def perspective_views_of_a_panorama(spherical_shot, width: int, reconstruction, image_format: str, rig_instance_count: Iterator[int]) -> List:
    """Create 6 perspective views of a panorama."""
    camera = Camera.create_perspective(0.5, 0.0, 0.0)
    camera.id = "perspective_panorama_camera"
    camera.width = width
    camera.height = width
    reconstruction.add_camera(camera)

    rig_instance = reconstruction.add_rig_instance(RigInstance(str(next(rig_instance_count))))
    shots = []
    for name, rotation in zip(PANORAMA_VIEW_NAMES, panorama_view_rotations()):
        if name not in reconstruction.rig_cameras:
            rig_camera_pose = Pose()
            rig_camera_pose.set_rotation_matrix(rotation)
            reconstruction.add_rig_camera(RigCamera(name, rig_camera_pose))
        rig_camera = reconstruction.rig_cameras[name]
        shot_id = add_image_format_extension(f"{spherical_shot.id}_perspective_view_{name}", image_format)
        shot = reconstruction.create_shot(shot_id, camera.id, Pose(), rig_camera.id, rig_instance.id)
        shot.metadata = spherical_shot.metadata
        shots.append(shot)
    rig_instance.pose = spherical_shot.pose
    return shots


def _view_rotation(panoshot, perspectiveshot) -> np.ndarray:
    return np.dot(panoshot.pose.get_rotation_matrix(), perspectiveshot.pose.get_rotation_matrix().T)


def render_perspective_views_of_a_panorama(image: np.ndarray, panoshot, perspectiveshots: Sequence, interpolation: int = INTER_LINEAR,
                                           border=BORDER_WRAP, out_sizes=None) -> List[np.ndarray]:
    """``render_perspective_view_of_a_panorama`` for every view of one panorama: the maps come from ``osfm_panorama_mapping`` (one call),
    the colours from ``osfm_remap_images`` (one call)"""
    views = [(s.camera, _view_rotation(panoshot, s)) for s in perspectiveshots]
    maps, _ = panorama_mappings(panoshot.camera, views, image.shape[1], image.shape[0])
    return remap_raw([image] * len(views), maps, interpolation, border, out_sizes)[0]


def undistort_image(shot, undistorted_shots: Sequence, original: Optional[np.ndarray], interpolation: int, max_size: int) -> Dict[str, np.ndarray]:
    """Undistort an image into a set of undistorted ones: ``{undistorted shot id: array}``, ``scale_image(max_size)`` applied.

    interpolation: ``INTER_AREA`` (images; cv2.remap treats it as linear) or ``INTER_NEAREST`` (masks, segmentations).  A panorama
    must already have the size ``4 w x 2 w`` of the views' width w: cv2's INTER_AREA resize is not restated here (ValueError otherwise)."""
    if original is None:
        return {}
    projection_type = shot.camera.projection_type
    if projection_type in FRAME_PROJECTIONS:
        [undistorted_shot] = undistorted_shots
        original = _image(original)
        height, width = original.shape[:2]
        outs, _ = undistort_raw([original], [0], [shot.camera], [undistorted_shot.camera], interpolation, [scale_image_size(height, width, max_size)])
        return {undistorted_shot.id: outs[0]}
    if projection_type in PANORAMA_PROJECTIONS:
        original = _image(original)
        subshot_width = undistorted_shots[0].camera.width
        width = 4 * subshot_width
        height = width // 2
        if original.shape[:2] != (height, width):
            raise ValueError(f"the panorama must be resized to {width} x {height} by the caller (cv2's INTER_AREA resize is out of scope); "
                             f"it is {original.shape[1]} x {original.shape[0]}")
        mint = INTER_LINEAR if interpolation == INTER_AREA else interpolation
        sizes = [scale_image_size(s.camera.height, s.camera.width, max_size) for s in undistorted_shots]
        outs = render_perspective_views_of_a_panorama(original, shot, undistorted_shots, mint, BORDER_WRAP, sizes)
        return {s.id: out for s, out in zip(undistorted_shots, outs)}
    raise NotImplementedError("Undistort not implemented for projection type: {}".format(shot.camera.projection_type))


def undistort_images(shots: Sequence, images: Sequence[Optional[np.ndarray]], masks: Optional[Sequence[Optional[np.ndarray]]] = None,
                     segmentations: Optional[Sequence[Optional[np.ndarray]]] = None, max_size: int = 100000,
                     undistorted_cameras: Optional[Sequence] = None) -> List[Dict[str, Optional[np.ndarray]]]:
    """The batch a driver uses for frame cameras -- what ``undistort_image_and_masks`` does shot by shot: one ``osfm_undistort_images``
    call per kind (images linear, masks and segmentations nearest) over a camera table without duplicates.  Returns, per shot,
    ``{"image": ..., "mask": ..., "segmentation": ...}`` (None where nothing was given).  undistorted_cameras: the undistorted shots'
    cameras (default ``undistorted_camera(shot.camera)``)."""
    table: Dict[tuple, int] = {}
    from_cameras, to_cameras, cam_of = [], [], []
    for k, shot in enumerate(shots):
        if shot.camera.projection_type not in FRAME_PROJECTIONS:
            raise NotImplementedError("Undistort not implemented for projection type: {}".format(shot.camera.projection_type))
        to_camera = undistorted_cameras[k] if undistorted_cameras is not None else undistorted_camera(shot.camera)
        key = tuple((m, p.tobytes()) for m, p in (camera_parameters(shot.camera), camera_parameters(to_camera)))
        if key not in table:
            table[key] = len(from_cameras)
            from_cameras.append(shot.camera)
            to_cameras.append(to_camera)
        cam_of.append(table[key])
    results: List[Dict[str, Optional[np.ndarray]]] = [{"image": None, "mask": None, "segmentation": None} for _ in shots]
    for kind, arrays, interpolation in (("image", images, INTER_AREA), ("mask", masks, INTER_NEAREST), ("segmentation", segmentations, INTER_NEAREST)):
        if arrays is None:
            continue
        which = [k for k, a in enumerate(arrays) if a is not None]
        batch = [_image(arrays[k]) for k in which]
        sizes = [scale_image_size(a.shape[0], a.shape[1], max_size) for a in batch]
        outs, _ = undistort_raw(batch, [cam_of[k] for k in which], from_cameras, to_cameras, interpolation, sizes)
        for k, out in zip(which, outs):
            results[k][kind] = out
    return results
