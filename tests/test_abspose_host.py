"""The absolute-pose LO-RANSAC of resect (opensfm_amd/csrc/abspose_core.h), compiled for the host with loops in place of lanes
(tests/native/abspose_host.cpp): the quartic against a 50-digit evaluation of the same formulas; the three-point and n-point solvers on
exact data with the reference's bounds; the header's walk (speculation, batched local optimisation) against an independent sequential
restatement of Estimate<RansacScoring, AbsolutePose> on this toolchain's std::mt19937, bit for bit; where the reference is mounted, the
reference's own robust_estimator.h around the same model numerics; resect's chord test against its numpy lines; and a stand-alone
program of the walk under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import abspose_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "opensfm_amd", "csrc")
REF = "/root/reference/opensfm"
OUT = os.path.join(HERE, "native", "_build")
HEADERS = ("abspose_core.h", "relrot_core.h", "loransac_walk.h", "relpose_core.h", "relpose_rounds.h")
THRESHOLD = 0.004


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def _compile(name, src, flags, shared=True):
    os.makedirs(OUT, exist_ok=True)
    target = os.path.join(OUT, name)
    deps = [src, os.path.join(HERE, "native", "abspose_host.cpp"), os.path.join(HERE, "native", "loop_wave.h")] + [os.path.join(CSRC, h) for h in HEADERS]
    if not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", *(["-fPIC", "-shared"] if shared else []), *flags,
                               "-o", target, src])
    return target


class Result(C.Structure):  # abspose_core.h AbsposeOut == osfm_abspose_result
    _fields_ = [("model", C.c_double * 12), ("lo_model", C.c_double * 12), ("score", C.c_int32), ("iterations", C.c_int32),
                ("num_inliers", C.c_int32)]


def build_host():
    lib = C.CDLL(_compile("abspose_host.so", os.path.join(HERE, "native", "abspose_host.cpp"), []))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.host_quartic.restype = C.c_int
    lib.host_quartic.argtypes = [dp, dp]
    lib.host_p3p_coefficients.restype = C.c_int
    lib.host_p3p_coefficients.argtypes = [dp, dp, dp]
    lib.host_p3p_models.restype = C.c_int
    lib.host_p3p_models.argtypes = [dp, dp, dp]
    lib.host_npoints_model.restype = None
    lib.host_npoints_model.argtypes = [dp, dp, C.c_int, dp]
    lib.host_abspose_error.restype = C.c_double
    lib.host_abspose_error.argtypes = [dp, dp, dp]
    lib.host_abspose_chord.restype = C.c_double
    lib.host_abspose_chord.argtypes = [dp, dp, dp]
    lib.host_abspose_images.restype = C.c_int
    lib.host_abspose_images.argtypes = [dp, dp, C.POINTER(C.c_int64), C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]
    lib.host_sequential_estimate.restype = C.c_int
    lib.host_sequential_estimate.argtypes = [dp, dp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, ip, ip, ip]
    return lib


@pytest.fixture(scope="module")
def host():
    return build_host()


def host_images(lib, b, X, off, threshold, probability=0.99, iterations=1000, use_lo=1, lo_iterations=10, use_reduction=1):
    """abspose_core.h's walk on the host: (list of Result, RANSAC mask, chord mask)"""
    b = np.ascontiguousarray(b, np.float64)
    X = np.ascontiguousarray(X, np.float64)
    off = np.ascontiguousarray(off, np.int64)
    n_images = len(off) - 1
    res = (Result * max(n_images, 1))()
    rmask, cmask = np.zeros(max(int(off[-1]), 1), np.uint8), np.zeros(max(int(off[-1]), 1), np.uint8)
    rc = lib.host_abspose_images(_p(b), _p(X), _p(off, C.c_int64), n_images, threshold, probability, iterations, use_lo, lo_iterations,
                                 use_reduction, C.cast(res, C.c_void_p), _p(rmask, C.c_uint8), _p(cmask, C.c_uint8))
    assert rc == 0, rc
    return [res[p] for p in range(n_images)], rmask[: int(off[-1])].astype(bool), cmask[: int(off[-1])].astype(bool)


def host_images_threads(lib, b, X, off, threshold, threads=16, **kw):
    """host_images with the images split over `threads` threads (the walk releases the GIL in ctypes): the same result"""
    import concurrent.futures as cf

    off = np.ascontiguousarray(off, np.int64)
    chunks = [ch for ch in np.array_split(np.arange(len(off) - 1), threads) if len(ch)]

    def run(ch):
        lo, hi = int(off[ch[0]]), int(off[ch[-1] + 1])
        return host_images(lib, b[lo:hi], X[lo:hi], off[ch[0]: ch[-1] + 2] - lo, threshold, **kw)

    with cf.ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(run, chunks))
    return [r for part in parts for r in part[0]], np.concatenate([part[1] for part in parts]), np.concatenate([part[2] for part in parts])


def sequential(lib, b, X, threshold, probability=0.99, iterations=1000, use_lo=1, lo_iterations=10, use_reduction=1, stats=None):
    b = np.ascontiguousarray(b, np.float64)
    X = np.ascontiguousarray(X, np.float64)
    n = len(b)
    m, lo, inl, it = np.zeros(12), np.zeros(12), np.zeros(max(n, 1), np.int32), np.zeros(1, np.int32)
    stats = np.zeros(2, np.int32) if stats is None else stats
    s = lib.host_sequential_estimate(_p(b), _p(X), n, threshold, probability, iterations, use_lo, lo_iterations, use_reduction, _p(m), _p(lo),
                                     _p(inl, C.c_int32), _p(it, C.c_int32), _p(stats, C.c_int32))
    return s, m, lo, inl[:s].copy(), int(it[0])


def same_bits(a, b):
    """equal as bit patterns (a model may hold NaN)"""
    return np.array_equal(np.ascontiguousarray(a, np.float64).ravel().view(np.int64), np.ascontiguousarray(b, np.float64).ravel().view(np.int64))


# ---- 1. the quartic ----
# Largest relative deviation of a refined, well-conditioned real root from the 50-digit evaluation, measured over the sets below:
# 2.3e-14.  The bound is 100 x that, the project's practice.
QUARTIC_MEASURED = 2.3e-14
QUARTIC_TOLERANCE = 100 * QUARTIC_MEASURED
# The order of the unrefined roots: a root moves by up to eps^(1/3) = 6e-6 at a triple root, the worst conditioning among the sets; 1e-4
# leaves a margin of 16 and is far below the distance between roots that a tie between models could depend on.  It is relative to the
# largest root of the set: the four roots are sums of the same terms (-b, Q7, the last square roots), so that is the size their
# rounding errors have (the cubic in disguise, alpha4 below epsilon, has a root near -4.5e15 and loses the other three before refinement).
ORDER_TOLERANCE = 1e-4


def _coefficients(lib):
    def of_sample(b, X):
        c = np.zeros(5)
        ok = lib.host_p3p_coefficients(_p(np.ascontiguousarray(b[:3])), _p(np.ascontiguousarray(X[:3])), _p(c))
        return c if ok else None

    return cases.p3p_coefficient_sets(of_sample)


def test_quartic_against_mpmath(host):
    import mpmath as mp

    sets = _coefficients(host)
    assert len(sets) >= 2000
    borderline = refused = compared = 0
    worst = 0.0
    for k, c in enumerate(sets):
        want, near_cut = cases.quartic_mp(c)
        got = np.zeros(8)
        ok = host.host_quartic(_p(np.ascontiguousarray(c)), _p(got))
        if near_cut:
            borderline += 1
            continue
        if want is None:
            assert ok == 0, k
            refused += 1
            continue
        assert ok == 1, k
        scale = 1 + max(abs(float(w)) for w in want)  # every root is a sum of terms up to the size of the largest one
        for j in range(4):  # the order: every unrefined root next to its counterpart
            assert abs(got[j] - float(want[j])) <= ORDER_TOLERANCE * scale, (k, j, got[:4], [float(w) for w in want])
        refined = cases.refine_mp(c, want)
        cm = [mp.mpf(float(v)) for v in c]
        for j in range(4):
            x = refined[j]
            p = (((cm[4] * x + cm[3]) * x + cm[2]) * x + cm[1]) * x + cm[0]
            dp = 4 * cm[4] * x**3 + 3 * cm[3] * x**2 + 2 * cm[2] * x + cm[1]
            size = sum(abs(cm[i] * x**i) for i in range(5))
            # a real root (the 50-digit iteration has converged on a zero of the polynomial), simple and well conditioned
            if x == 0 or abs(p) > mp.mpf("1e-40") * size or size > 1e3 * abs(x * dp):
                continue
            dev = float(abs(mp.mpf(float(got[4 + j])) - x) / abs(x))
            worst = max(worst, dev)
            compared += 1
            assert dev <= QUARTIC_TOLERANCE, (k, j, dev)
    print(f"quartic: {len(sets)} sets, {borderline} branch-borderline, {refused} refused, {compared} well-conditioned real roots, "
          f"largest relative deviation {worst:.3e}")
    assert borderline <= 0.01 * len(sets)  # the seed keeps the 50-digit evaluation itself under the cap
    assert refused >= 2 and compared >= 2000


def test_principal_cube_and_square_roots(host):
    """the arithmetic-only roots against 50-digit principal roots, the negative real axis and both sides of it included.  Bound: 8 eps of
    the modulus -- the unit part's last Newton step, the modulus and their product each round a few times, nothing accumulates"""
    import mpmath as mp

    mp.mp.dps = 50
    rng = np.random.default_rng(6)
    zs = [complex(*rng.normal(0, 10.0 ** rng.integers(-8, 8), 2)) for _ in range(2000)]
    zs += [complex(-2.0, 0.0), complex(-2.0, 1e-13), complex(-2.0, -1e-13), complex(3.0, 0.0), complex(0.0, 5.0), complex(0.0, -5.0), 1e-300 + 0j,
           complex(-1e10, 1e-5), complex(1e300, -1e300), 0j]
    bound = 8 * 2.0 ** -52
    for z in zs:
        zin, out = np.array([z.real, z.imag]), np.zeros(2)
        zm = mp.mpc(z.real, z.imag)
        for k, fn in ((3, host.host_ccbrt), (2, host.host_csqrt)):
            fn(_p(zin), _p(out))
            want = mp.mpc(0) if z == 0 else mp.exp(mp.log(zm) / k)
            assert abs(mp.mpc(out[0], out[1]) - want) <= bound * abs(want), (z, k, out, want)


# ---- 2. the solvers on exact data ----
def test_three_points_on_exact_data(host):
    """test_multiview.py::test_absolute_pose_three_points restaged: one of the models within 1e-6 (Frobenius) in all but at most 2 shots"""
    shots = cases.exact_shots()
    exact_found = 0
    for Rt, b, X in shots:
        models = np.zeros(48)
        count = host.host_p3p_models(_p(b), _p(X), _p(models))
        assert count == 4
        for m in models.reshape(4, 3, 4):
            exact_found += bool(np.linalg.norm(Rt - m, ord="fro") < 1e-6)
    assert exact_found >= len(shots) - 2


def test_n_points_on_exact_data(host):
    """test_multiview.py::test_absolute_pose_n_points restaged: within 1e-5 (Frobenius) on every shot"""
    for Rt, b, X in cases.exact_shots():
        model = np.zeros(12)
        host.host_npoints_model(_p(b), _p(X), len(b), _p(model))
        assert np.linalg.norm(Rt - model.reshape(3, 4), ord="fro") < 1e-5


def test_degenerate_samples_give_no_model(host):
    rng = np.random.default_rng(3)
    b, X, _, _ = cases.make_problem(rng, 3, "exact")
    models = np.zeros(48)
    dup_b, dup_X = b.copy(), X.copy()
    dup_b[1], dup_X[1] = dup_b[0], dup_X[0]  # duplicate points: k1 = 0, sigma == 0
    assert host.host_p3p_models(_p(dup_b), _p(dup_X), _p(models)) == 0
    line_X = np.ascontiguousarray(np.array([[0.0, 0.0, 5.0], [1.0, 0.0, 5.0], [2.0, 0.0, 5.0]]))  # collinear points: u1 x k1 = 0
    assert host.host_p3p_models(_p(b), _p(line_X), _p(models)) == 0
    flat_b = np.ascontiguousarray(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.6, 0.8, 0.0]]))  # b3 in the plane of b1, b2: k3 . b3 == 0
    assert host.host_p3p_models(_p(flat_b), _p(X), _p(models)) == 0


# ---- 3. the walk ----
@pytest.fixture(scope="module")
def walked(host):
    """the problem set and the header's walk over it, computed once for the tests that compare it"""
    probs = cases.problem_set(n_max=2000)
    b, X, off = cases.pack(probs)
    res, mask, _ = host_images(host, b, X, off, THRESHOLD)
    return probs, off, res, mask


def test_walk_equals_sequential_estimate_bit_for_bit(host, walked):
    probs, off, res, mask = walked
    assert len(probs) >= 150
    early = 0
    stats = np.zeros(2, np.int32)
    for k, (pb, pX, _, _) in enumerate(probs):
        s, m, lo, inl, it = sequential(host, pb, pX, THRESHOLD, stats=stats)
        r = res[k]
        assert r.score == s, k
        assert r.iterations == it, k
        assert same_bits(np.array(r.model), m) and same_bits(np.array(r.lo_model), lo), k
        assert np.array_equal(np.flatnonzero(mask[off[k]: off[k + 1]]), inl), k
        early += it < 1000
    assert early >= 20        # early stops occur
    assert stats[0] >= 1      # a local-optimisation iteration improved the best
    assert stats[1] >= 1      # a sample without a model occurred


@pytest.mark.parametrize("use_lo,lo_iterations,use_reduction,iterations,probability",
                         [(0, 10, 1, 1000, 0.99), (1, 3, 1, 200, 0.999), (1, 10, 0, 120, 0.99), (1, 0, 1, 1000, 0.5), (1, 70, 1, 60, 0.99)])
def test_walk_equals_sequential_estimate_other_parameters(host, use_lo, lo_iterations, use_reduction, iterations, probability):
    probs = cases.problem_set(seed=3, count=36, n_max=800, sizes=[3, 5, 6, 24, 64, 65])
    b, X, off = cases.pack(probs)
    res, mask, _ = host_images(host, b, X, off, 0.006, probability, iterations, use_lo, lo_iterations, use_reduction)
    for k, (pb, pX, _, _) in enumerate(probs):
        s, m, lo, inl, it = sequential(host, pb, pX, 0.006, probability, iterations, use_lo, lo_iterations, use_reduction)
        assert (res[k].score, res[k].iterations) == (s, it), k
        assert same_bits(np.array(res[k].model), m) and same_bits(np.array(res[k].lo_model), lo), k
        assert np.array_equal(np.flatnonzero(mask[off[k]: off[k + 1]]), inl), k


# ---- 4. against the reference's own template, where it is mounted ----
need_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference is not mounted")


@need_ref
def test_walk_equals_reference_estimator_template(host, walked):
    ref = C.CDLL(_compile("abspose_ref.so", os.path.join(HERE, "native", "abspose_ref_adapter.cpp"),
                          ["-I", os.path.join(ROOT, "oracle", "ref_adapters", "stubs"), "-I", os.path.join(REF, "src", "robust")]))
    ref.ref_ransac_absolute_pose.restype = C.c_int
    probs, off, res, mask = walked
    for k, (pb, pX, _, _) in enumerate(probs):
        m, lo, inl = np.zeros(12), np.zeros(12), np.zeros(len(pb), np.int32)
        s = ref.ref_ransac_absolute_pose(_p(pb), _p(pX), len(pb), C.c_double(THRESHOLD), 1000, C.c_double(0.99), 1, 10, 1, _p(m), _p(lo),
                                         _p(inl, C.c_int32))
        assert res[k].score == s, k
        if s > 0:  # (with no inlier at all the reference's models are uninitialised)
            assert same_bits(np.array(res[k].model), m) and same_bits(np.array(res[k].lo_model), lo), k
        assert np.array_equal(np.flatnonzero(mask[off[k]: off[k + 1]]), inl[:s]), k


# ---- 5. the chord tail ----
def test_chord_tail_against_numpy(host):
    rng = np.random.default_rng(5)
    probs = [cases.make_problem(rng, n, kind, outliers=o) for n, kind, o in
             [(60, "exact", 0.0), (300, "noisy", 0.5), (200, "planar", 0.1), (50, "noisy", 0.35), (800, "behind", 0.2), (4097, "noisy", 0.6)]]
    b, X, off = cases.pack(probs)
    res, _, cmask = host_images(host, b, X, off, THRESHOLD)
    borderline = 0
    for k, (bs, Xs, _, _) in enumerate(probs):
        Rt = np.array(res[k].lo_model).reshape(3, 4)  # multiview.py:487-491
        R, t = Rt[:3, :3].copy(), Rt[:, 3].copy()
        T = Rt.copy()
        T[:3, :3] = R.T
        T[:, 3] = -R.T.dot(t)
        R, t = T[:, :3], T[:, 3]  # reconstruction.py:727-733
        reprojected_bs = R.T.dot((Xs - t).T).T
        reprojected_bs /= np.linalg.norm(reprojected_bs, axis=1)[:, np.newaxis]
        d = np.linalg.norm(reprojected_bs - bs, axis=1)
        inliers = d < THRESHOLD
        near = np.abs(d - THRESHOLD) <= 8 * np.spacing(THRESHOLD)
        borderline += int(near.sum())
        got = cmask[off[k]: off[k + 1]]
        assert np.array_equal(got[~near], inliers[~near]), k
        assert abs(res[k].num_inliers - int(inliers.sum())) <= int(near.sum()), k
        assert res[k].num_inliers == int(got.sum())
    assert borderline <= 2


def test_error_and_chord_operation_order(host):
    rng = np.random.default_rng(4)
    for _ in range(100):
        M = np.ascontiguousarray(np.c_[cases.rotation(rng, 1.0), rng.normal(size=3)])
        b, X = np.ascontiguousarray(rng.normal(size=3)), np.ascontiguousarray(rng.normal(size=3) * 3)
        v = [((M[r, 0] * X[0] + M[r, 1] * X[1]) + M[r, 2] * X[2]) + M[r, 3] for r in range(3)]
        nb = np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
        nv = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        bn, vn = [x / nb for x in b], [x / nv for x in v]
        e = 1.0 - ((bn[0] * vn[0] + bn[1] * vn[1]) + bn[2] * vn[2])
        assert host.host_abspose_error(_p(M), _p(b), _p(X)) == e


# ---- 6. a stand-alone program under the sanitizers ----
def test_standalone_walk_under_sanitizers():
    exe = _compile("abspose_main", os.path.join(HERE, "native", "abspose_main.cpp"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                   shared=False)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "abspose_main: ok" in done.stdout
