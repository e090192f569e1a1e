"""An independent restatement of ``dense::DepthmapPruner::Prune`` (opensfm/src/dense/src/depthmap.cc:565-625) in numpy -- float32 where the
reference uses float, float64 where it uses double, its order of operations -- and the fixtures the pruning tests share.  NOT the
product: nothing under opensfm_amd/ imports it, and it was written from depthmap.cc, not from prune_core.h.

Vectorised over the pixels of view 0: the rule is elementwise, so the rounding is that of the scalar code, and boolean indexing keeps
the raster order of the reference's push_back.  ``cv::normalize`` and the Matx product order are restated from memory of OpenCV, as in
``depthmap_cases``: the squares summed in double in index order, a square root, each product with ``nv ? 1. / nv : 0.`` in double and
rounded to float."""
import numpy as np

from depthmap_cases import D, F, camera, clean_problem, inverse3, matvec, render, rotation  # noqa: F401 -- shared vocabulary

TALLY = ("behind", "outside", "not_above", "zero_depth", "area_rejected", "area_survived", "truncated_to_zero")
I64_LIMIT = 2147483648.0  # |x / z + 0.5| from here on, or NaN: outside the image (the two divergences of include/osfm_mi355.h)


def normalize(v):
    """cv::normalize of N Vec3f"""
    vd = v.astype(D)
    s = ((D(0) + vd[:, 0] * vd[:, 0]) + vd[:, 1] * vd[:, 1]) + vd[:, 2] * vd[:, 2]
    nv = np.sqrt(s)
    with np.errstate(all="ignore"):
        scale = np.where(nv != 0, D(1) / nv, D(0))
    return (vd * scale[:, None]).astype(F)


def empty_cloud():
    return np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros((0, 3), np.uint8), np.zeros(0, np.uint8)


def prune(views, threshold):
    """views: [(K, R, t, depth, plane, color, label), ...] -> (points, normals, colors, labels), tally of the branches (and, under
    "kept", the flat indices of the kept pixels of view 0 in raster order)"""
    K = [np.asarray(v[0], D).reshape(3, 3) for v in views]
    R = [np.asarray(v[1], D).reshape(3, 3) for v in views]
    t = [np.asarray(v[2], D).reshape(3) for v in views]
    depths = [np.ascontiguousarray(v[3], F) for v in views]
    planes = [np.ascontiguousarray(v[4], F) for v in views]
    tally = dict.fromkeys(TALLY, 0)
    h, w = depths[0].shape
    if h * w == 0:
        tally["kept"] = np.zeros(0, np.int64)
        return empty_cloud(), tally
    I, J = [a.reshape(-1) for a in np.mgrid[0:h, 0:w]]
    depth = depths[0].reshape(-1)
    with np.errstate(all="ignore"):
        live = ~(depth <= 0)  # `if (depth <= 0) continue;`: a NaN stays
        normal = normalize(planes[0].reshape(-1, 3))
        area = ((-normal[:, 2] / depth).astype(D) * K[0][0, 0]).astype(F)
        S = inverse3(K[0])[None] * depth.astype(D)[:, None, None]
        q = matvec(S, np.stack([J.astype(D), I.astype(D), np.ones(len(I), D)], 1)) - t[0][None]
        point = matvec(np.ascontiguousarray(R[0].T)[None], q).astype(F)
        keep = live.copy()
        bound = D(F(1) - F(threshold))
        for o in range(1, len(views)):
            ho, wo = depths[o].shape
            rp = matvec(K[o][None], matvec(R[o][None], point.astype(D)) + t[o][None])
            z = rp[:, 2]
            seen = live & ~((z < 1e-8) | np.isnan(z))
            ru, rv = rp[:, 0] / z + D(0.5), rp[:, 1] / z + D(0.5)
            castable = (np.abs(ru) < I64_LIMIT) & (np.abs(rv) < I64_LIMIT)
            iu = np.where(castable, np.trunc(np.where(castable, ru, 0)), -1).astype(np.int64)
            iv = np.where(castable, np.trunc(np.where(castable, rv, 0)), -1).astype(np.int64)
            inside = seen & castable & (iv >= 0) & (iv < ho) & (iu >= 0) & (iu < wo)
            cu, cv = np.where(inside, iu, 0), np.where(inside, iv, 0)
            if ho * wo:
                depth_at = depths[o][cv, cu]
                normal_at = normalize(planes[o][cv, cu])
            else:
                depth_at, normal_at = np.zeros(len(I), F), np.zeros((len(I), 3), F)
            above = inside & (depth_at.astype(D) > bound * z)
            zero = above & (depth_at == 0)
            larger = (-normal_at[:, 2] / depth_at).astype(D) * K[o][0, 0] > area.astype(D)
            rejected = above & ~zero & larger
            keep &= ~(zero | rejected)
            tally["behind"] += int(np.count_nonzero(live & ~seen))
            tally["outside"] += int(np.count_nonzero(seen & ~inside))
            tally["not_above"] += int(np.count_nonzero(inside & ~above))
            tally["zero_depth"] += int(np.count_nonzero(zero))
            tally["area_rejected"] += int(np.count_nonzero(rejected))
            tally["area_survived"] += int(np.count_nonzero(above & ~zero & ~larger))
            tally["truncated_to_zero"] += int(np.count_nonzero(inside & ((ru < 0) | (rv < 0))))
        Rinv = np.ascontiguousarray(R[0].T).astype(F)
        rotated = (Rinv[None, :, 0] * normal[:, None, 0] + Rinv[None, :, 1] * normal[:, None, 1]) + Rinv[None, :, 2] * normal[:, None, 2]
    tally["kept"] = np.flatnonzero(keep)
    colors = np.ascontiguousarray(views[0][5], np.uint8).reshape(-1, 3)
    labels = np.ascontiguousarray(views[0][6], np.uint8).reshape(-1)
    return (point[keep], rotated[keep].astype(F), colors[keep], labels[keep]), tally


def live_pixels(views):
    with np.errstate(all="ignore"):
        return int(np.count_nonzero(~(np.asarray(views[0][3], F) <= 0)))


# ---- fixtures ----
def plane_of(k, h, w):
    i, j = np.mgrid[0:h, 0:w].astype(D)
    frac = np.mod(np.sin((37 * i + 91 * j + 13 * k) * 12.9898) * 43758.5453, 1.0)
    return np.stack([0.3 * np.sin(0.7 * i + k), 0.3 * np.cos(0.9 * j - k), -(0.6 + 0.4 * frac)], -1).astype(F)


def color_of(k, h, w):
    i, j = np.mgrid[0:h, 0:w]
    return np.stack([(7 * i + 3 * j + 50 * c + k) % 256 for c in range(3)], -1).astype(np.uint8)


def label_of(h, w):
    i, j = np.mgrid[0:h, 0:w]
    return ((i + 2 * j) % 7).astype(np.uint8)


def dress(views):
    """(K, R, t, depth) of every view -> (K, R, t, depth, plane, color, label)"""
    out = []
    for k, (K, R, t, depth) in enumerate(views):
        h, w = depth.shape
        out.append((K, R, t, depth, plane_of(k, h, w), color_of(k, h, w), label_of(h, w)))
    return out


def prune_problem(n_views=3, w=37, h=29, behind=True):
    return {"views": dress(clean_problem(n_views, w, h, behind)["views"])}


def first_view_problem(w, h, n_views=3):
    """a first view of w x h at the origin (rendered depth, zeros as in clean_problem) in front of clean_problem's other views"""
    K = camera(w, h)
    depth = render(K, np.eye(3), np.zeros(3), w, h)[1].astype(F)
    depth[::5, ::7] = 0
    return {"views": dress([(K, np.eye(3), np.zeros(3), depth)] + clean_problem(n_views, 37, 29, False)["views"][1:])}


def with_depth(problem, view, depth):
    views = list(problem["views"])
    views[view] = views[view][:3] + (np.ascontiguousarray(depth, F),) + views[view][4:]
    return {"views": views}


def nan_problem():
    p = prune_problem(3, 37, 29, True)
    depth = p["views"][0][3].copy()
    depth[4, 9] = depth[11, 3] = np.nan
    return with_depth(p, 0, depth)


def overflow_problem():
    """the second view's principal point at 1e12: every x / z + 0.5 of it is past 2^31 (divergence 1)"""
    p = prune_problem(3, 37, 29, False)
    views = list(p["views"])
    K = np.array(views[1][0], D)
    K[0, 2] = 1e12
    views[1] = (K,) + views[1][1:]
    return {"views": views}


def single_view_problem():
    return {"views": prune_problem(3, 37, 29, True)["views"][:1]}


def zero_first_problem():
    p = prune_problem(3, 37, 29, True)
    return with_depth(p, 0, np.zeros_like(p["views"][0][3]))


# name -> (problem, threshold): what tests/test_prune_host.py and tests/test_gpu_prune.py compare byte for byte
FIXTURES = {
    "t001_behind": (lambda: prune_problem(3, 37, 29, True), 0.01),
    "t001_front": (lambda: prune_problem(3, 37, 29, False), 0.01),
    "t150_behind": (lambda: prune_problem(3, 37, 29, True), 1.5),
    "t150_front": (lambda: prune_problem(3, 37, 29, False), 1.5),
}
MORE = {
    "five_views": (lambda: prune_problem(5, 64, 48, True), 0.01),
    "single_view": (single_view_problem, 0.01),
    "zero_first": (zero_first_problem, 0.01),
    "one_pixel": (lambda: first_view_problem(1, 1), 0.01),
    "one_row": (lambda: first_view_problem(300, 1), 0.01),
    "nan_depth": (nan_problem, 0.01),
    "overflow": (overflow_problem, 0.01),
}
_PROBLEMS, _EXPECTED = {}, {}


def problem(name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = {**FIXTURES, **MORE}[name][0]()
    return _PROBLEMS[name]


def threshold(name):
    return {**FIXTURES, **MORE}[name][1]


def expected(name):
    """the restatement's (cloud, tally) of a case, computed once per process"""
    if name not in _EXPECTED:
        _EXPECTED[name] = prune(problem(name)["views"], threshold(name))
    return _EXPECTED[name]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_cloud(got, want):
    """byte equality of the four arrays, shapes and dtypes included"""
    return len(got) == 4 and all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def concatenate(clouds):
    return tuple(np.concatenate([c[k] for c in clouds]) for k in range(4))
