"""Inputs shared by the absolute-pose tests (tests/test_abspose_host.py on the CPU, tests/test_gpu_abspose.py on the GPU): resection
problems of every kind the walk has a path for, exact shots for the solver leaves, quartic coefficient sets, and the 50-digit
evaluation of the quartic formula."""
import numpy as np

# the sizes at which the walk changes path: the LO sample size (6, 24), the wave edge (63 .. 65), the LDS inlier list (4096, 4097)
SIZES = [3, 4, 5, 6, 7, 23, 24, 25, 63, 64, 65, 128, 1000, 4096, 4097]
KINDS = ("exact", "noisy", "planar", "behind", "all_outliers", "duplicates")


def rotation(rng, scale=0.3):
    r = rng.normal(0, scale, 3)
    th = np.linalg.norm(r)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / max(th, 1e-300)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_problem(rng, n, kind="noisy", outliers=0.3, noise=1e-3):
    """(bearings, points, R, t) of one image: n rows, x_cam = R X + t.  kind: exact (no noise, no outliers), noisy, planar (all points on
    a plane), behind (a third of the points behind the camera: their bearings point backwards), all_outliers, duplicates (a fifth of the
    rows repeat other rows, so that samples with two equal points -- sigma == 0, no model -- occur)"""
    R = rotation(rng)
    t = rng.normal(0, 1, 3)
    Xc = np.c_[rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)]
    if kind == "planar":
        Xc[:, 2] = 6.0 + 0.3 * Xc[:, 0] - 0.2 * Xc[:, 1]
    if kind == "behind":
        Xc[rng.random(n) < 0.33, 2] *= -1.0
    X = (Xc - t) @ R  # R^T (x_cam - t)
    b = Xc / np.linalg.norm(Xc, axis=1, keepdims=True)
    if kind != "exact":
        b = b + rng.normal(0, noise, b.shape)
        frac = 1.0 if kind == "all_outliers" else outliers
        bad = rng.random(n) < frac
        v = rng.normal(size=(int(bad.sum()), 3))
        b[bad] = v
        b /= np.linalg.norm(b, axis=1, keepdims=True)
    if kind == "duplicates" and n > 1:
        count = max(1, n // 5)
        src, dst = rng.integers(0, n, count), rng.integers(0, n, count)
        b[dst], X[dst] = b[src], X[src]
    return np.ascontiguousarray(b), np.ascontiguousarray(X), R, t


def problem_set(seed=0, count=150, n_max=5000, sizes=SIZES):
    """~count problems: SIZES once, the rest log-uniform in [3, n_max]; the kinds in turn; outlier fractions 0 - 90 %"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = sizes[k] if k < len(sizes) else int(np.exp(rng.uniform(np.log(3), np.log(n_max))))
        kind = KINDS[(k + k // len(KINDS)) % len(KINDS)]
        out.append(make_problem(rng, n, kind, outliers=rng.uniform(0.0, 0.9), noise=rng.choice([2e-4, 1e-3])))
    return out


def pack(probs):
    b = np.concatenate([p[0] for p in probs])
    X = np.concatenate([p[1] for p in probs])
    off = np.r_[0, np.cumsum([len(p[0]) for p in probs])].astype(np.int64)
    return b, X, off


def exact_shots(seed=2, count=40, n=60):
    """the data of the reference's shots_and_their_points fixture, restaged: (world-to-camera 3 x 4, bearings, points) of `count` shots
    with exact bearings"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        b, X, R, t = make_problem(rng, n, "exact")
        out.append((np.c_[R, t], b, X))
    return out


# ---- the quartic ----
def p3p_coefficient_sets(host_coefficients, seed=4, count=1990):
    """[c0 .. c4] of the quartic of `count` random P3P samples (host_coefficients: bearings (3, 3), points (3, 3) -> coefficients or None)
    plus hand-made sets: a double root, alpha4 below epsilon, all four discriminant terms below epsilon, complex pairs"""
    rng = np.random.default_rng(seed)
    sets = []
    while len(sets) < count:
        b, X, _, _ = make_problem(rng, 3, "exact" if len(sets) % 2 else "noisy", outliers=0.0)
        c = host_coefficients(b, X)
        if c is not None:
            sets.append(c)
    hand = [
        np.poly([0.5, 0.5, -0.3, 0.8])[::-1],            # a double root
        np.poly([0.25, 0.25, 0.25, -0.7])[::-1] * 3.0,   # a triple root
        np.r_[np.poly([0.2, -0.4, 0.9])[::-1], 1e-17],   # alpha4 below epsilon: a cubic in disguise
        np.array([0.0, 0.0, 0.0, 0.0, 1.0]),             # x^4: Q1 .. Q4 all zero, SolveQuartic returns false
        np.array([1e-20, 0.0, 0.0, 0.0, 1.0]),           # still below epsilon
        np.poly([0.3 + 0.4j, 0.3 - 0.4j, -0.6, 0.1]).real[::-1],             # one complex pair
        np.poly([0.3 + 0.4j, 0.3 - 0.4j, -0.2 + 0.7j, -0.2 - 0.7j]).real[::-1],  # two complex pairs
        np.poly([0.1 + 1e-3j, 0.1 - 1e-3j, 0.5, -0.5]).real[::-1] * 0.01,    # a nearly real pair
        np.poly([1.0, -1.0, 0.5, -0.5])[::-1],            # symmetric: b = d = 0
        np.poly([0.9, 0.1, -0.1, -0.9])[::-1] * 1e3,
    ]
    return sets + [np.ascontiguousarray(h, np.float64) for h in hand]


def quartic_mp(coefficients, cut_tolerance=1e-12):
    """foundation::SolveQuartic evaluated with mpmath at 50 digits, principal branches (exp(log(z) / k) with arg in (-pi, pi]).
    -> (roots or None where it returns false, borderline).  borderline: a complex intermediate whose root is extracted lies within
    cut_tolerance (relative) of the branch cut, the negative real axis, without lying on it exactly -- the side it falls on is then a
    matter of rounding.  That covers the argument of the cube root and of Q7's square root, and the discriminant Q2^2 / 4 - Q1^3 when
    it cancels to within cut_tolerance (its sign picks the branch).  A real intermediate (an imaginary part of exactly zero) has one
    principal root; the last two square roots contribute their real parts only, which are continuous across the cut."""
    import mpmath as mp

    mp.mp.dps = 50
    eps = mp.mpf(2) ** -52
    c0, c1, c2, c3, c4 = [mp.mpf(float(v)) for v in coefficients]
    a = c4 if abs(c4) > eps else eps
    b, c, d, e = c3 / a, c2 / a, c1 / a, c0 / a
    Q1 = c * c - 3 * b * d + 12 * e
    Q2 = 2 * c * c * c - 9 * b * c * d + 27 * d * d + 27 * b * b * e - 72 * c * e
    Q3 = 8 * b * c - 16 * d - 2 * b * b * b
    Q4 = 3 * b * b - 8 * c
    if abs(Q1) < eps and abs(Q2) < eps and abs(Q3) < eps and abs(Q4) < eps:
        return None, False

    def near_cut(z):
        z = mp.mpc(z)
        return z.real < 0 and z.imag != 0 and abs(z.imag) <= cut_tolerance * abs(z)

    def root(z, k):
        z = mp.mpc(z)
        if z == 0:
            return mp.mpc(0)
        return mp.exp(mp.log(z) / k)

    D = Q2 * Q2 / 4 - Q1 * Q1 * Q1
    borderline = abs(D) <= cut_tolerance * max(abs(Q2 * Q2 / 4), abs(Q1 * Q1 * Q1))
    z5 = Q2 / 2 + root(D, 2)
    borderline = borderline or near_cut(z5)
    Q5 = root(z5, 3)
    if Q5 == 0:
        return None, True
    Q6 = (Q1 / Q5 + Q5) / 3
    z7 = Q4 / 12 + Q6
    borderline = borderline or near_cut(z7)
    Q7 = 2 * root(z7, 2)
    if Q7 == 0:
        return None, True
    sm = root(4 * Q4 / 6 - 4 * Q6 - Q3 / Q7, 2)
    sp = root(4 * Q4 / 6 - 4 * Q6 + Q3 / Q7, 2)
    roots = [(-b - Q7 - sm).real / 4, (-b - Q7 + sm).real / 4, (-b + Q7 - sp).real / 4, (-b + Q7 + sp).real / 4]
    return roots, bool(borderline)


def refine_mp(coefficients, roots, steps=5):
    """RefineQuarticRoots at 50 digits"""
    import mpmath as mp

    c = [mp.mpf(float(v)) for v in coefficients]
    out = []
    for x in roots:
        for _ in range(steps):
            f = (((c[4] * x + c[3]) * x + c[2]) * x + c[1]) * x + c[0]
            df = 4 * c[4] * x**3 + 3 * c[3] * x**2 + 2 * c[2] * x + c[1]
            decr = 0 if df == 0 else f / df
            if abs(decr) < mp.mpf("1e-20"):
                break
            x = x - decr
        out.append(x)
    return out
