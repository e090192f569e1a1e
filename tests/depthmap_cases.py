"""An independent restatement of ``dense::DepthmapEstimator`` and ``dense::DepthmapCleaner`` (opensfm/src/dense/src/depthmap.cc) in numpy --
float32 where the reference uses float, float64 where it uses double, its order of operations -- and the synthetic scenes the depthmap
tests share.  NOT the product: nothing under opensfm_amd/ imports it, and it builds no table of its own (``tables`` come from
``osfm_depthmap_tables``).  The PatchMatch sweeps are the reference's plain sequential raster loops, NOT wavefronts.

Vectorisation is over candidates only (N planes of N pixels, or one plane in N views): every float sum keeps the reference's order --
``np.add.accumulate`` is sequential by definition."""
import hashlib
import os

import numpy as np

F = np.float32
D = np.float64
M64 = (1 << 64) - 1
QUANTILES, KR2 = 4096, 99
BRUTE_FORCE, PATCH_MATCH, PATCH_MATCH_SAMPLE = 0, 1, 2


# ---- cv::Matx as remembered: products summed k = 0, 1, 2; the inverse by cofactors times the reciprocal determinant ----
def inverse3(a):
    a = np.asarray(a, D).reshape(9)
    d = a[0] * (a[4] * a[8] - a[7] * a[5]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6])
    d = D(1.0) / d
    return np.array([(a[4] * a[8] - a[5] * a[7]) * d, (a[2] * a[7] - a[1] * a[8]) * d, (a[1] * a[5] - a[2] * a[4]) * d,
                     (a[5] * a[6] - a[3] * a[8]) * d, (a[0] * a[8] - a[2] * a[6]) * d, (a[2] * a[3] - a[0] * a[5]) * d,
                     (a[3] * a[7] - a[4] * a[6]) * d, (a[1] * a[6] - a[0] * a[7]) * d, (a[0] * a[4] - a[1] * a[3]) * d], D).reshape(3, 3)


def matmul(A, B):
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + A[..., :, 2, None] * B[..., None, 2, :]


def matvec(A, x):
    return (A[..., :, 0] * x[..., None, 0] + A[..., :, 1] * x[..., None, 1]) + A[..., :, 2] * x[..., None, 2]


class Estimator:
    """the state AddView builds: Kinv of view 0, K, Q = R R_0^T, a = Q t_0 - t per view, images, the mask of view 0"""

    def __init__(self, views, tables, patch_size=7, min_patch_sd=1.0):
        self.K = [np.asarray(v[0], D).reshape(3, 3) for v in views]
        R = [np.asarray(v[1], D).reshape(3, 3) for v in views]
        t = [np.asarray(v[2], D).reshape(3) for v in views]
        self.images = [np.ascontiguousarray(v[3], np.uint8) for v in views]
        self.mask = np.ascontiguousarray(views[0][4], np.uint8)
        self.Kinv = inverse3(self.K[0])
        self.Q = [matmul(r, np.ascontiguousarray(R[0].T)) for r in R]
        self.a = [matvec(q, t[0]) - tt for q, tt in zip(self.Q, t)]
        self.n = len(views)
        self.h, self.w = self.images[0].shape
        self.patch_size = patch_size
        self.hpz = (patch_size - 1) // 2
        self.min_patch_variance = F(min_patch_sd) * F(min_patch_sd)
        self.tables = tables
        r = np.arange(-self.hpz, self.hpz + 1)
        self.DY, self.DX = np.repeat(r, patch_size), np.tile(r, patch_size)  # dy then dx
        self.depth = np.zeros((self.h, self.w), F)
        self.plane = np.zeros((self.h, self.w, 3), F)
        self.score = np.zeros((self.h, self.w), F)
        self.nghbr = np.zeros((self.h, self.w), np.int32)

    # PlaneFromDepthAndNormal, N at once
    def plane_from_depth_normal(self, x, y, depth, normal):
        S = self.Kinv[None] * depth.astype(D)[:, None, None]
        xy1 = np.stack([x.astype(D), y.astype(D), np.ones(len(x), D)], 1)
        p = matvec(S, xy1).astype(F)
        denom = -((normal[:, 0] * p[:, 0] + normal[:, 1] * p[:, 1]) + normal[:, 2] * p[:, 2])
        inv = F(1) / np.where(denom > F(1e-6), denom, F(1e-6))
        return normal * inv[:, None]

    # DepthOfPlaneBackprojection
    def depth_of_plane(self, x, y, plane):
        v = plane.astype(D)
        r = (v[:, 0, None] * self.Kinv[None, 0, :] + v[:, 1, None] * self.Kinv[None, 1, :]) + v[:, 2, None] * self.Kinv[None, 2, :]
        denom = (-((r[:, 0] * x.astype(D) + r[:, 1] * y.astype(D)) + r[:, 2] * D(1.0))).astype(F)
        return F(1) / np.where(denom > F(1e-6), denom, F(1e-6))

    def sample_coordinates(self, i, j, plane, other):
        """w, x2, y2 of lines 433-459 for N (pixel, plane, view) triples: (N,), (N, patch area), (N, patch area)"""
        Q = np.stack([self.Q[o] for o in other])
        a = np.stack([self.a[o] for o in other])
        K = np.stack([self.K[o] for o in other])
        M = Q + a[:, :, None] * plane.astype(D)[:, None, :]
        H = matmul(matmul(K, M), self.Kinv[None]).astype(F)
        fi, fj = i.astype(F), j.astype(F)
        with np.errstate(all="ignore"):
            u = (H[:, 0, 0] * fj + H[:, 0, 1] * fi) + H[:, 0, 2]
            v = (H[:, 1, 0] * fj + H[:, 1, 1] * fi) + H[:, 1, 2]
            w = (H[:, 2, 0] * fj + H[:, 2, 1] * fi) + H[:, 2, 2]
            ww = w * w
            dfdx_x = (H[:, 0, 0] * w - H[:, 2, 0] * u) / ww
            dfdx_y = (H[:, 1, 0] * w - H[:, 2, 0] * v) / ww
            dfdy_x = (H[:, 0, 1] * w - H[:, 2, 1] * u) / ww
            dfdy_y = (H[:, 1, 1] * w - H[:, 2, 1] * v) / ww
            Hx0, Hy0 = u / w, v / w
            DXf, DYf = self.DX.astype(F)[None], self.DY.astype(F)[None]
            x2 = (Hx0[:, None] + dfdx_x[:, None] * DXf) + dfdy_x[:, None] * DYf
            y2 = (Hy0[:, None] + dfdx_y[:, None] * DXf) + dfdy_y[:, None] * DYf
        return w, x2, y2

    # ComputePlaneImageScore for N (pixel, plane, view) triples
    def image_score(self, i, j, plane, other):
        N = len(i)
        w, x2, y2 = self.sample_coordinates(i, j, plane, other)
        with np.errstate(all="ignore"):
            im0 = self.images[0]
            p = im0[i[:, None] + self.DY[None], j[:, None] + self.DX[None]].astype(np.int64)
            center = im0[i, j].astype(np.int64)
            wt = self.tables["weight"][np.abs(p - center[:, None]), (self.DX * self.DX + self.DY * self.DY)[None]]
            im1 = p.astype(F)
            im2 = np.zeros((N, len(self.DX)), F)
            for o in set(int(q) for q in other):
                rows = np.nonzero(other == o)[0]
                im2[rows] = interpolate(self.images[o], y2[rows], x2[rows])

            value = ncc(im1, im2, wt)
        return np.where(w == 0, F(-1), value).astype(F)

    # ComputePlaneScore for ONE pixel and plane: the strict > keeps the lowest view on a tie
    def plane_score(self, i, j, plane):
        score, nghbr = F(-1), 0
        if self.n > 1:
            others = np.arange(1, self.n)
            s = self.image_score(np.full(self.n - 1, i), np.full(self.n - 1, j), np.repeat(plane[None], self.n - 1, 0), others)
            for o, value in zip(others, s):
                if value > score:
                    score, nghbr = value, int(o)
        return score, nghbr

    def assign(self, i, j, depth, plane, score, nghbr):
        self.depth[i, j], self.plane[i, j], self.score[i, j], self.nghbr[i, j] = depth, plane, score, nghbr

    def check(self, i, j, plane, score, nghbr):
        if score > self.score[i, j]:
            depth = self.depth_of_plane(np.array([j]), np.array([i]), plane[None])[0]
            self.assign(i, j, depth, plane, score, nghbr)

    def interior(self):
        return [(i, j) for i in range(self.hpz, self.h - self.hpz) for j in range(self.hpz, self.w - self.hpz)]

    # ---- ComputeBruteForce ----
    def brute_force(self, min_depth, max_depth, num_planes):
        pix = self.interior()
        if not pix:
            return self.result()
        I, J = np.array([p[0] for p in pix]), np.array([p[1] for p in pix])
        normal = np.tile(np.array([0, 0, -1], F), (len(pix), 1))
        for d in range(num_planes):
            if num_planes <= 1:
                depth = F(min_depth)
            else:
                depth = F(D(1) / (D(1) / D(min_depth) + D(d) * (D(1) / D(max_depth) - D(1) / D(min_depth)) / D(num_planes - 1)))
            plane = self.plane_from_depth_normal(J, I, np.full(len(pix), depth, F), normal)
            score, nghbr = np.full(len(pix), -1, F), np.zeros(len(pix), np.int32)
            for o in range(1, self.n):
                s = self.image_score(I, J, plane, np.full(len(pix), o))
                better = s > score
                score, nghbr = np.where(better, s, score), np.where(better, o, nghbr)
            better = score > self.score[I, J]
            new_depth = self.depth_of_plane(J, I, plane)
            for q in np.nonzero(better)[0]:
                self.assign(I[q], J[q], new_depth[q], plane[q], score[q], nghbr[q])
        return self.result()

    # ---- PatchMatch ----
    def sample_mode(self, method):
        return method == PATCH_MATCH_SAMPLE and self.n > 1

    def random_initialization(self, method, seed, init_depth):
        for i, j in self.interior():
            local = i * self.w + j
            depth = init_depth[draw_bits(seed, 0, local, 0) >> 52]
            normal = np.array([uniform_pm1(draw_bits(seed, 0, local, 1)), uniform_pm1(draw_bits(seed, 0, local, 2)), -1], F)
            plane = self.plane_from_depth_normal(np.array([j]), np.array([i]), np.array([depth], F), normal[None])[0]
            if self.sample_mode(method):
                nghbr = 1 + ((draw_bits(seed, 0, local, 3) >> 32) & 0xFFFFFFFF) % (self.n - 1)
                score = self.image_score(np.array([i]), np.array([j]), plane[None], np.array([nghbr]))[0]
            else:
                score, nghbr = self.plane_score(i, j, plane)
            self.assign(i, j, depth, plane, score, nghbr)

    def patch_variance(self, i, j):
        x = self.images[0][i - self.hpz:i + self.hpz + 1, j - self.hpz:j + self.hpz + 1].astype(F).reshape(-1)
        n = self.patch_size * self.patch_size
        mean = np.add.accumulate(x, dtype=F)[-1] / F(n)
        return np.add.accumulate((x - mean) * (x - mean), dtype=F)[-1] / F(n)

    def ignore_mask(self):
        for i, j in self.interior():
            if self.mask[i, j] == 0 or self.patch_variance(i, j) < self.min_patch_variance:
                self.assign(i, j, F(0), np.zeros(3, F), F(0), 0)

    def check_image(self, i, j, plane, nghbr):
        self.check(i, j, plane, self.image_score(np.array([i]), np.array([j]), plane[None], np.array([nghbr]))[0], nghbr)

    def check_plane(self, i, j, plane):
        score, nghbr = self.plane_score(i, j, plane)
        self.check(i, j, plane, score, nghbr)

    def update_pixel(self, state, i, j, adjacent, sample, seed, sweep):
        """PatchMatchUpdatePixel; `state` is what adjacent pixels are read from (the estimator itself in the reference)"""
        if self.depth[i, j] == 0:
            return
        local = i * self.w + j
        T = self.tables
        for di, dj in adjacent:
            ia, ja = i + di, j + dj
            if state.depth[ia, ja] == 0:
                continue
            plane = state.plane[ia, ja].copy()
            if sample:
                self.check_image(i, j, plane, int(state.nghbr[ia, ja]))
            else:
                self.check_plane(i, j, plane)
        depth_range, normal_range = F(0.02), F(0.5)
        current_nghbr = int(self.nghbr[i, j])
        for k in range(6):
            depth = self.depth[i, j] * T["factor"][k, draw_bits(seed, sweep, local, 3 * k) >> 52]
            cp = self.plane[i, j].copy()
            if cp[2] != 0:
                assert depth_range == depth_range_of(k)
                normal = np.array([-cp[0] / cp[2] + normal_range * T["normal"][draw_bits(seed, sweep, local, 3 * k + 1) >> 52],
                                   -cp[1] / cp[2] + normal_range * T["normal"][draw_bits(seed, sweep, local, 3 * k + 2) >> 52], -1], F)
                plane = self.plane_from_depth_normal(np.array([j]), np.array([i]), np.array([depth], F), normal[None])[0]
                if sample:
                    self.check_image(i, j, plane, current_nghbr)
                else:
                    self.check_plane(i, j, plane)
                depth_range = F(D(depth_range) * D(0.3))
                normal_range = F(D(normal_range) * D(0.8))
            # (a plane with a zero third entry `continue`s past the two range updates in the reference; it cannot occur: the third
            # entry of every plane assigned to an unignored pixel is -1 / max(1e-6, denom))
        if not sample or self.n <= 2:
            return
        off = ((draw_bits(seed, sweep, local, 18) >> 32) & 0xFFFFFFFF) % (self.n - 2)
        other = 1 + (current_nghbr + off) % (self.n - 1)
        self.check_image(i, j, self.plane[i, j].copy(), other)

    def post_process(self):
        padded = np.pad(self.depth, 2, mode="edge")
        windows = np.stack([padded[a:a + self.h, b:b + self.w] for a in range(5) for b in range(5)], -1)
        m = np.sort(windows, -1)[..., 12]
        with np.errstate(all="ignore"):
            bad = (self.depth == 0) | ((np.abs(self.depth - m) / self.depth).astype(D) > 0.05)
        self.depth[bad] = 0

    def patch_match(self, method, min_depth, max_depth, iterations, seed, init_depth, propagate=True):
        """`propagate=False`: every pixel of a pass reads its adjacent pixels as they were BEFORE the pass (not the reference: the test
        that the order matters)"""
        if not self.interior():
            return self.result()
        sample = self.sample_mode(method)
        self.random_initialization(method, seed, init_depth)
        self.ignore_mask()
        for it in range(iterations):
            for backward in (False, True):
                sweep = 1 + 2 * it + int(backward)
                adjacent = ((0, 1), (1, 0)) if backward else ((-1, 0), (0, -1))
                order = self.interior()
                state = self if propagate else Snapshot(self)
                for i, j in (reversed(order) if backward else order):
                    self.update_pixel(state, i, j, adjacent, sample, seed, sweep)
        self.post_process()
        return self.result()

    def result(self):
        return self.depth, self.plane, self.score, self.nghbr


def ncc(x, y, w):
    """NCCEstimator: Push over the last axis in order, then Get"""
    def seq(a):
        return np.add.accumulate(a, axis=-1, dtype=F)[..., -1]

    with np.errstate(all="ignore"):
        sumx, sumy = seq(w * x), seq(w * y)
        sumxx, sumyy, sumxy = seq((w * x) * x), seq((w * y) * y), seq((w * x) * y)
        sumw = seq(w)
        meanx, meany = sumx / sumw, sumy / sumw
        meanxx, meanyy, meanxy = sumxx / sumw, sumyy / sumw, sumxy / sumw
        varx, vary = meanxx - meanx * meanx, meanyy - meany * meany
        value = (meanxy - meanx * meany) / np.sqrt(varx * vary)
        minus = (sumw == 0) | (varx.astype(D) < 0.1) | (vary.astype(D) < 0.1)
    return np.where(minus, F(-1), value).astype(F)


def plane_induced_homography(K1, R1, t1, K2, R2, t2, v):
    """PlaneInducedHomography (depthmap.cc:88-94), in double"""
    R2R1 = matmul(R2, np.ascontiguousarray(R1.T))
    return matmul(matmul(K2, R2R1 + (matvec(R2R1, t1) - t2)[:, None] * v[None, :]), inverse3(K1))


def project(x, K, R, t):
    return matvec(K, matvec(R, x) + t)


def backproject(x, y, depth, K, R, t):
    return matvec(np.ascontiguousarray(R.T), matvec(inverse3(K) * D(depth), np.array([x, y, 1.0])) - t)


class Snapshot:
    def __init__(self, e):
        self.depth, self.plane, self.nghbr = e.depth.copy(), e.plane.copy(), e.nghbr.copy()


def depth_range_of(k):
    r = F(0.02)
    for _ in range(k):
        r = F(D(r) * D(0.3))
    return r


# LinearInterpolation<T>; a NaN coordinate reads as 0
def interpolate(image, y, x):
    rows, cols = image.shape
    if rows < 2 or cols < 2:
        return np.zeros(x.shape, F)
    ok = (x >= 0) & (x < F(cols - 1)) & (y >= 0) & (y < F(rows - 1))
    xs, ys = np.where(ok, x, F(0)), np.where(ok, y, F(0))
    ix, iy = xs.astype(np.int64), ys.astype(np.int64)
    dx, dy = xs - ix.astype(F), ys - iy.astype(F)
    im00, im01 = image[iy, ix].astype(F), image[iy, ix + 1].astype(F)
    im10, im11 = image[iy + 1, ix].astype(F), image[iy + 1, ix + 1].astype(F)
    im0 = (F(1) - dx) * im00 + dx * im01
    im1 = (F(1) - dx) * im10 + dx * im11
    return np.where(ok, (F(1) - dy) * im0 + dy * im1, F(0)).astype(F)


# ---- the draws (include/osfm_mi355.h) ----
def draw_bits(seed, sweep, pixel, k):
    z = (seed + 0x9E3779B97F4A7C15 * ((((sweep << 40) + pixel) * 32 + k + 1) & M64)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def uniform_pm1(z):
    return F(z >> 40) * F(2.0 ** -23) - F(1)


def estimate(problem, method, tables, init_depth=None, patch_size=7, iterations=3, num_planes=100, min_patch_sd=1.0, seed=0, propagate=True):
    """one problem ({"views", "min_depth", "max_depth"}) -> depth, plane, score, nghbr"""
    views = problem["views"]
    h, w = np.asarray(views[0][3]).shape
    hpz = (patch_size - 1) // 2
    if h - 2 * hpz < 1 or w - 2 * hpz < 1:
        return np.zeros((h, w), F), np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), np.int32)
    e = Estimator(views, tables, patch_size, min_patch_sd)
    if method == BRUTE_FORCE:
        return e.brute_force(problem["min_depth"], problem["max_depth"], num_planes)
    return e.patch_match(method, problem["min_depth"], problem["max_depth"], iterations, seed, init_depth, propagate)


# ---- DepthmapCleaner::Clean ----
def clean(views, threshold, min_consistent):
    K = [np.asarray(v[0], D).reshape(3, 3) for v in views]
    R = [np.asarray(v[1], D).reshape(3, 3) for v in views]
    t = [np.asarray(v[2], D).reshape(3) for v in views]
    depths = [np.ascontiguousarray(v[3], F) for v in views]
    h, w = depths[0].shape
    if h * w == 0:
        return np.zeros((h, w), F)
    I, J = [a.reshape(-1) for a in np.mgrid[0:h, 0:w]]
    depth = depths[0].reshape(-1)
    S = inverse3(K[0])[None] * depth.astype(D)[:, None, None]
    q = matvec(S, np.stack([J.astype(D), I.astype(D), np.ones(len(I), D)], 1)) - t[0][None]
    point = matvec(np.ascontiguousarray(R[0].T)[None], q).astype(F).astype(D)
    consistent = np.ones(len(I), np.int64)
    with np.errstate(all="ignore"):
        for o in range(1, len(views)):
            rp = matvec(K[o][None], matvec(R[o][None], point) + t[o][None]).astype(F)
            skip = (rp[:, 2].astype(D) < 1e-8) | np.isnan(rp[:, 2])
            u, v = rp[:, 0] / rp[:, 2], rp[:, 1] / rp[:, 2]
            at = interpolate(depths[o], v[:, None], u[:, None])[:, 0]
            same = np.abs(at - rp[:, 2]) < rp[:, 2] * F(threshold)
            consistent += (~skip & same)
    return np.where(consistent >= min_consistent, depth, F(0)).astype(F).reshape(h, w)


# ---- synthetic scenes ----
def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def texture(x, y):
    """procedural, in world coordinates of a surface; one flat patch (x in [-1.5, -0.4], y in [-1.3, -0.1])"""
    cell = np.floor(x * 5.0) * 7919.0 + np.floor(y * 5.0) * 104729.0
    noise = np.mod(np.sin(cell * 12.9898) * 43758.5453, 1.0)
    v = 128.0 + 45.0 * np.sin(9.0 * x + 2.0 * y) + 35.0 * np.sin(13.0 * y - 4.0 * x + 1.0) + 60.0 * (noise - 0.5)
    flat = (x > -1.5) & (x < -0.4) & (y > -1.3) & (y < -0.1)
    return np.where(flat, 128.0, v)


X_STEP, Z_NEAR, Z_FAR, SLANT = 0.35, 4.0, 5.0, 0.25  # z = Z_NEAR + SLANT x for x < X_STEP, Z_FAR + SLANT x beyond, a wall between


def render(K, R, t, w, h):
    """the image and the depth (z in the camera) of the scene by exact ray casting: the slanted plane, the step and the wall between"""
    K, R, t = np.asarray(K, D).reshape(3, 3), np.asarray(R, D).reshape(3, 3), np.asarray(t, D).reshape(3)
    if w * h == 0:
        return np.zeros((h, w), np.uint8), np.zeros((h, w), D)
    jj, ii = np.meshgrid(np.arange(w, dtype=D), np.arange(h, dtype=D))
    rays = (R.T @ (np.linalg.inv(K) @ np.stack([jj.ravel(), ii.ravel(), np.ones(w * h)]))).T  # world directions, z = 1 in the camera
    origin = -R.T @ t
    best = np.full(w * h, np.inf)
    value = np.zeros(w * h)
    with np.errstate(all="ignore"):
        for z0, side in ((Z_NEAR, -1), (Z_FAR, 1)):
            s = (z0 + SLANT * origin[0] - origin[2]) / (rays[:, 2] - SLANT * rays[:, 0])
            X = origin[None] + s[:, None] * rays
            ok = (s > 0) & ((X[:, 0] < X_STEP) if side < 0 else (X[:, 0] >= X_STEP)) & (s < best)
            best, value = np.where(ok, s, best), np.where(ok, texture(X[:, 0], X[:, 1]), value)
        s = (X_STEP - origin[0]) / rays[:, 0]
        X = origin[None] + s[:, None] * rays
        ok = (s > 0) & (X[:, 2] >= Z_NEAR + SLANT * X_STEP) & (X[:, 2] <= Z_FAR + SLANT * X_STEP) & (s < best)
        best, value = np.where(ok, s, best), np.where(ok, texture(X[:, 2] + 3.0, X[:, 1]), value)
    image = np.clip(np.rint(np.where(np.isfinite(best), value, 0.0)), 0, 255).astype(np.uint8).reshape(h, w)
    return image, np.where(np.isfinite(best), best, 0.0).reshape(h, w)


def camera(w, h):
    f = 0.9 * max(w, h, 1)
    return np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1.0]])


def make_problem(w, h, n_views, sizes=None, duplicate=False, outside=False, baseline=0.25):
    """view 0 at the origin; the others on a baseline with small rotations.  `sizes`: (w, h) of the other views; `duplicate`: the last view
    repeats view 1 (a tie); `outside`: the last view keeps its (non-zero) rendered image but its principal point moves to
    (-5000, 7000), so every sample of every plane lands left of and below the image: LinearInterpolation's bounds test gives the zeros.  The texture's cells are about two
    pixels wide at these focal lengths: the images are point-sampled, and finer detail would alias differently in every view"""
    views, truth = [], None
    for k in range(n_views):
        wk, hk = (w, h) if k == 0 or sizes is None else sizes[(k - 1) % len(sizes)]
        if k == 0:
            R, c = np.eye(3), np.zeros(3)
        else:
            side = 1 if k % 2 else -1
            R = rotation(0.01 * k, -0.03 * side * ((k + 1) // 2), 0.005 * k)
            c = np.array([baseline * side * ((k + 1) // 2), 0.04 * (k - 2), 0.02 * k])
        if duplicate and k == n_views - 1 and k > 1:
            views.append(tuple(np.copy(a) for a in views[1]))
            continue
        K = camera(wk, hk)
        t = -R @ c
        image, depth = render(K, R, t, wk, hk)
        if k == 0:
            truth = depth
        if outside and k == n_views - 1 and k > 0:
            K = K.copy()
            K[0, 2], K[1, 2] = -5000.0, 7000.0
        mask = np.full((hk, wk), 255, np.uint8)
        if k == 0 and hk > 6 and wk > 6:
            mask[hk // 2:hk // 2 + 4, 2:7] = 0  # a zero block
        views.append((K, R, t, image, mask))
    return {"views": views, "min_depth": 3.0, "max_depth": 6.5, "truth": truth}


# name -> (problem arguments, estimator arguments): the shapes of tests/test_gpu_depthmap.py and tests/test_depthmap_host.py
CASES = {
    "wide_3views_p7": (dict(w=40, h=32, n_views=3), dict(patch_size=7, iterations=1, num_planes=8)),
    "tall_3views_p5": (dict(w=33, h=47, n_views=3), dict(patch_size=5, iterations=2, num_planes=8)),
    "wide_2views_p3": (dict(w=40, h=32, n_views=2), dict(patch_size=3, iterations=1, num_planes=8)),
    "patch_sized": (dict(w=7, h=7, n_views=3), dict(patch_size=7, iterations=1, num_planes=8)),
    "below_patch": (dict(w=6, h=9, n_views=3), dict(patch_size=7, iterations=1, num_planes=8)),
    "single_view": (dict(w=20, h=17, n_views=1), dict(patch_size=5, iterations=1, num_planes=8)),
    "other_sizes": (dict(w=33, h=29, n_views=3, sizes=((41, 23), (20, 37))), dict(patch_size=5, iterations=1, num_planes=8)),
    "duplicate_view": (dict(w=31, h=27, n_views=3, duplicate=True), dict(patch_size=5, iterations=1, num_planes=8)),
    "all_outside": (dict(w=31, h=27, n_views=3, outside=True), dict(patch_size=5, iterations=1, num_planes=8)),
    "one_plane": (dict(w=29, h=23, n_views=3), dict(patch_size=5, iterations=1, num_planes=1)),
    "five_views": (dict(w=64, h=48, n_views=5), dict(patch_size=7, iterations=1, num_planes=8)),
}
METHOD_NAMES = {BRUTE_FORCE: "brute_force", PATCH_MATCH: "patch_match", PATCH_MATCH_SAMPLE: "patch_match_sample"}
SEED = 20240607
_PROBLEMS, _EXPECTED = {}, {}


def problem(name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = make_problem(**CASES[name][0])
    return _PROBLEMS[name]


GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depthmap")


def tables_digest(tables, init_depth):
    h = hashlib.sha256()
    for a in (tables["normal"], tables["factor"], tables["weight"], init_depth):
        h.update(np.ascontiguousarray(a, F).tobytes())
    return h.hexdigest()


def golden(name, method, tables, init_depth):
    """the stored result of the restatement (tests/golden/gen_depthmap_golden.py), or None when there is none for these tables"""
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    if not os.path.exists(path):
        return None
    with np.load(path) as z:
        if str(z["tables_digest"]) != tables_digest(tables, init_depth):
            return None
        return tuple(z[f"{METHOD_NAMES[method]}_{k}"] for k in ("depth", "plane", "score", "nghbr"))


def expected(name, method, tables, init_depth, fresh=False):
    """the restatement's result for a case: the stored one unless `fresh`, else computed, once per process"""
    key = (name, method)
    if not fresh:
        stored = golden(name, method, tables, init_depth)
        if stored is not None:
            return stored
    if key not in _EXPECTED:
        _EXPECTED[key] = estimate(problem(name), method, tables, init_depth, seed=SEED, **CASES[name][1])
    return _EXPECTED[key]


def clean_problem(n_views=3, w=37, h=29, behind=True):
    """depthmaps with zeros, true depths elsewhere; the last view may sit behind the scene looking away"""
    views = []
    for k in range(n_views):
        wk, hk = (w, h) if k == 0 else (w + 3, h - 2)
        K = camera(wk, hk)
        side = 1 if k % 2 else -1
        R = np.eye(3) if k == 0 else rotation(0.01 * k, -0.03 * side, 0.0)
        c = np.zeros(3) if k == 0 else np.array([0.2 * side * ((k + 1) // 2), 0.03, 0.0])
        if behind and k == n_views - 1 and k > 0:
            R = rotation(0.0, np.pi, 0.0)
        t = -R @ c
        depth = render(K, R, t, wk, hk)[1].astype(F)
        depth[::5, ::7] = 0
        if k == 1:
            depth[3:9, 4:12] *= F(1.02)  # inconsistent with view 0
        views.append((K, R, t, depth))
    return {"views": views}
