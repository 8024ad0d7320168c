"""The cases of tests/test_sac_edges_cpu.py and tests/test_sac_edges_gpu.py: what tests/sac_cases.py does not reach.  Degenerate
three-pair samples (collinear sources, one target point, mirrored targets, sources an ulp apart), the edges of the stopping rule
(every pair an inlier, none, n = 3 .. 5, max_iterations 0 and 1, a probability whose log is 0, a run into a cut sixth batch,
seeds from 2^63 up), a list of 70 001 pairs, and the float32 range (the clouds and the threshold times 2^e, a cloud of denormals,
thresholds whose square is +inf, above FLT_MAX, below the least denormal, 0, or exactly a float).

What each case is FOR is asserted on the reference by tests/test_sac_edges_cpu.py; the GPU test compares bits.  Every cloud comes
from a fixed seed; the seeds of the rejector were picked so that the property holds and sac_ref.replay's k-margin is kept.
"""
import functools
import math

import numpy as np

import sac_cases as K
import sac_ref as R

FLT_MAX = np.float32(np.finfo(np.float32).max)
FLT_MIN = np.float32(np.finfo(np.float32).tiny)
N_A = 300
LINE_A, LINE_D = np.float32([0.5, -0.25, 1.0]), np.float32([0.125, 0.25, -0.125])


def moved(src):
    """MOTION applied in float64, rounded to float32 (sac_cases.motion_case's true pairs)"""
    return (np.asarray(src, np.float64) @ K.MOTION[:3, :3].T + K.MOTION[:3, 3]).astype(np.float32)


def identity_corr(n, seed=0):
    corr = np.zeros(n, K.CORR)
    corr["index_query"] = corr["index_match"] = np.arange(n)
    corr["distance"] = np.random.default_rng(seed).uniform(0, 100, n).astype(np.float32)
    return corr


def line(n=N_A, step=1.0, seed=0):
    """n distinct points LINE_A + k * step * LINE_D, k the integers -n/2 .. n/2 - 1 shuffled; step a power of two, so every
    coordinate is a dyadic number of a few bits and EXACT in float32: the points are collinear exactly"""
    k = (np.random.default_rng(seed).permutation(n) - n // 2).astype(np.float64) * step
    xyz = LINE_A.astype(np.float64) + k[:, None] * LINE_D.astype(np.float64)
    assert (xyz.astype(np.float32) == xyz).all()
    return xyz.astype(np.float32)


def collinear(share=1.0, seed=40):
    src = line(seed=seed)
    tgt = moved(src)
    rng = np.random.default_rng(seed)
    true = np.ones(N_A, bool)
    true[rng.permutation(N_A)[:N_A - int(round(share * N_A))]] = False
    tgt[~true] = rng.uniform(-3.5, 3.5, ((~true).sum(), 3)).astype(np.float32)
    return src, tgt, identity_corr(N_A, seed), true


def collinear_exact_turn(seed=41):
    """the line turned by 90 degrees about z and shifted by integers: exact in float32, so the targets are collinear exactly as well
    and a three-pair cross-covariance has rank 1 up to the rounding of its own few operations"""
    src = line(seed=seed)
    tgt = np.stack([-src[:, 1] + 3, src[:, 0] - 2, src[:, 2] + 1], axis=1).astype(np.float32)
    return src, tgt, identity_corr(N_A, seed), np.ones(N_A, bool)


def one_target(seed=42):
    """every pair names target record 7; the sources on a line, 1/256 of LINE_D apart"""
    src = line(step=1.0 / 32, seed=seed)
    tgt = np.random.default_rng(seed).uniform(-3.5, 3.5, (N_A, 3)).astype(np.float32)
    corr = identity_corr(N_A, seed)
    corr["index_match"] = 7
    return src, tgt, corr, None


def coplanar_mirrored(seed=43):
    """the targets are the sources reflected in the plane z = 0 (exact)"""
    src = np.random.default_rng(seed).uniform(-2, 2, (N_A, 3)).astype(np.float32)
    return src, (src * np.float32([1, 1, -1])).astype(np.float32), identity_corr(N_A, seed), None


def one_ulp_apart(scale_exp, seed=44):
    """source point i = 2^scale_exp * (1 + i * 2^-23, 0.5, -0.25), shuffled: neighbours differ in the last bit of x.  scale_exp 0: the
    squared distances are k^2 * 2^-46, tiny normal floats.  scale_exp -51: k^2 * 2^-148, positive float32 DENORMALS for every k < 300.
    The targets are the sources' exact MOTION image (at -51 all the same point: MOTION's translation)."""
    i = np.random.default_rng(seed).permutation(N_A).astype(np.float64)
    xyz = np.stack([1.0 + i * 2.0 ** -23, np.full(N_A, 0.5), np.full(N_A, -0.25)], axis=1) * 2.0 ** scale_exp
    assert (xyz.astype(np.float32) == xyz).all()
    src = xyz.astype(np.float32)
    return src, moved(src), identity_corr(N_A, seed), None


def prefix(n, seed=51):
    """the first n pairs of motion_case(300, share 1.0)"""
    src, tgt, corr, true = K.motion_case(300, 1.0, seed)
    return src, tgt, corr[:n], true[:n]


# ---- the large list
BIG_N = 70001
BIG_H = 4096
EXACT_N = K.TILE * (K.MAX_GROUPS // (BIG_H // K.CHUNK))        # 32 768 pairs: 64 tiles x 64 chunks = MAX_GROUPS workgroups exactly


def big():
    return K.motion_case(BIG_N, 0.5, 61)


def transforms_fast_pick(H, seed=0):
    """(the 331 distinct transforms of sac_cases.transforms_fast(H, seed), which of them each of its H rows is)"""
    return K.transforms(331, seed), np.random.default_rng(seed).integers(0, 331, H)


# ---- the float32 range
SCALE_EXPONENTS = (-100, -70, -62, -30, 30, 62, 70, 100)
SCALE_SEED, SCALE_IT = 71, 100


def scale_base():
    return K.motion_case(400, 0.5, 7)


def scaled(xyz, e):
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(np.asarray(xyz, np.float32), int(e)).astype(np.float32)


def scaled_case(e):
    src, tgt, corr, true = scale_base()
    return scaled(src, e), scaled(tgt, e), corr, true


def denormal_case():
    """scale_base() moved to positive coordinates, at 2^-140: every coordinate a float32 denormal"""
    src, tgt, corr, true = scale_base()
    s, t = scaled(src + np.float32(3.0), -140), scaled(tgt + np.float32(7.0), -140)
    assert (s > 0).all() and (s < FLT_MIN).all() and (t > 0).all() and (t < FLT_MIN).all()
    return s, t, corr, true


def scale_prm(e):
    return dict(seed=SCALE_SEED, max_iterations=SCALE_IT, inlier_threshold=math.ldexp(0.05, e))


# thresholds at scale 1 whose square is +inf in double, above FLT_MAX, below 2^-149, 0 in double
RANGE_THRESHOLDS = (1e200, 2e19, 1e-30, 1e-200)


def range_threshold_pairs():
    """(source xyz, target xyz, corr, d2 under the identity): pairs whose d2 is 0, the least denormal 2^-149, 2^-148, an ordinary
    float, a float just below FLT_MAX, +inf by overflow -- and one NaN pair"""
    root = np.float32(np.sqrt(2.0) * 2.0 ** -75)                                 # root * root = 2^-149 (1 - 2e-8), which rounds to 2^-149
    x = np.float32([0.0, 0.0, root, 2.0 ** -74, 2.0 ** -74, 0.25, 1.0, 1.8e19, 1.84e19, 1.85e19, 3e19, 3e38, np.nan])
    tgt = np.zeros((len(x), 3), np.float32)
    tgt[:, 0] = x
    tgt[4, 1] = np.float32(2.0 ** -74)                                          # 2^-148 + 2^-148
    tgt[1] = np.float32([3.0, -2.0, 0.5])
    src = np.zeros_like(tgt)
    src[1] = tgt[1]                                                             # d2 = 0 away from the origin
    d2 = R.l2_simple(src, tgt)
    return src, tgt, identity_corr(len(x)), d2


def extreme_transforms_case():
    """(source xyz, target xyz, corr, transforms): points at and near +-FLT_MAX, ordinary ones, denormals and zeros, against
    transforms that hold FLT_MAX, denormals and -0.0.  Products and sums overflow to +-inf on the way, and inf - inf gives NaN."""
    big, tiny = float(FLT_MAX), 2.0 ** -140
    vals = np.float32([big, -big, 0.75 * big, -0.5 * big, 1e30, -1e19, 1.5, -0.0, 0.0, tiny, -3 * tiny, 2.0 ** -126])
    rng = np.random.default_rng(81)
    src = vals[rng.integers(0, len(vals), (200, 3))]
    tgt = vals[rng.integers(0, len(vals), (200, 3))]
    tgt[:40] = src[:40]                                                         # (under the identity these have d2 = 0 or NaN (inf - inf) ...)
    Ts = np.zeros((14, 4, 4), np.float32)
    Ts[:] = np.eye(4)
    Ts[1, :3, :3] *= -0.0                                                       # the zero matrix with signs: 0 * FLT_MAX = 0, -0.0 + 0.0
    Ts[2, 0, :2] = big                                                          # FLT_MAX * x + FLT_MAX * y: +-inf, or inf - inf
    Ts[3, :3, 3] = (big, -big, big)                                             # x + FLT_MAX
    Ts[4, :3, :3] = np.float32([[0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    Ts[5, :3, :3] = tiny                                                        # denormal * x: a denormal or 0
    Ts[6, :3, :3], Ts[6, :3, 3] = 2.0, (-big, big, -big)                        # 2 x overflows, - FLT_MAX does not bring it back
    Ts[7, :3, :3] = np.float32([[2, 2, 0], [2, -2, 0], [0, 1, 1]])              # 2 x + 2 y: inf - inf across TWO products; y + z: inf from finite ones
    Ts[8, :3, :3] = 0.5
    Ts[9, :3, :3], Ts[9, :3, 3] = np.float32([[0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5]]), (tiny, -tiny, -0.0)
    Ts[10, :3, :3] = big                                                        # FLT_MAX * FLT_MAX
    Ts[11, 0, 0], Ts[11, 1, 1], Ts[11, 2, 2] = -0.0, tiny, -1.0
    Ts[12, :3, :3], Ts[12, :3, 3] = -0.0, tgt[3]
    Ts[13, :3, :3], Ts[13, :3, 3] = K.MOTION[:3, :3], K.MOTION[:3, 3]
    return src, tgt, identity_corr(200), Ts


def few_finite_case(finite_pairs, n=500, seed=91):
    """a list of n pairs of which exactly `finite_pairs` are finite: the others name a source or a target record that holds a NaN
    or an infinity"""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    tgt = moved(src)
    keep = np.sort(rng.permutation(n)[:finite_pairs])
    bad = np.setdiff1d(np.arange(n), keep)
    for j, i in enumerate(bad):
        (src if j % 2 else tgt)[i, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    return src, tgt, identity_corr(n, seed), keep


# the rejector's cases: name -> (case, parameters)
CASES = {
    # A. degenerate samples
    "collinear": (lambda: collinear(), dict(seed=101, max_iterations=100)),
    "collinear_exact_turn": (lambda: collinear_exact_turn(), dict(seed=102, max_iterations=100)),
    "collinear_noisy": (lambda: collinear(0.6), dict(seed=103, max_iterations=200)),
    "one_target": (lambda: one_target(), dict(seed=104, max_iterations=100)),
    "coplanar_mirrored": (lambda: coplanar_mirrored(), dict(seed=105, max_iterations=100)),
    "coincident_sources_apart_by_one_ulp": (lambda: one_ulp_apart(0), dict(seed=106, max_iterations=100)),
    "coincident_sources_apart_by_one_ulp_denormal_d2": (lambda: one_ulp_apart(-51), dict(seed=107, max_iterations=100)),
    # B. the stopping rule's edges
    "all_inliers": (lambda: K.motion_case(300, 1.0, 51), dict(seed=111, max_iterations=100)),
    "n3": (lambda: prefix(3), dict(seed=201, max_iterations=50)),
    "n3_threshold_zero": (lambda: prefix(3), dict(seed=201, max_iterations=50, inlier_threshold=0.0)),
    "n4": (lambda: prefix(4), dict(seed=113, max_iterations=50)),
    "n5": (lambda: prefix(5), dict(seed=114, max_iterations=50)),
    "threshold_zero": (lambda: K.motion_case(300, 0.5, 52), dict(seed=115, max_iterations=100, inlier_threshold=0.0)),
    "max_iterations_0": (lambda: K.motion_case(300, 0.5, 52), dict(seed=116, max_iterations=0)),
    "max_iterations_1": (lambda: K.motion_case(300, 0.5, 52), dict(seed=309, max_iterations=1)),
    "probability_1e-300": (lambda: K.motion_case(300, 0.5, 52), dict(seed=118, max_iterations=100, probability=1e-300, inlier_threshold=0.0)),
    "probability_1e-300_found": (lambda: K.motion_case(300, 0.5, 52), dict(seed=309, max_iterations=100, probability=1e-300)),
    "probability_0.9999999999999999": (lambda: K.motion_case(300, 1.0, 51), dict(seed=119, max_iterations=100, probability=0.9999999999999999)),
    "deep": (lambda: K.motion_case(1500, 0.1, 53), dict(seed=120, max_iterations=9000, probability=0.999999)),
    "seed_2^63": (lambda: K.motion_case(600, 0.5, 54), dict(seed=1 << 63, max_iterations=200)),
    "seed_2^64-3": (lambda: K.motion_case(600, 0.5, 54), dict(seed=(1 << 64) - 3, max_iterations=200)),
    # C. the large list
    "big": (lambda: big(), dict(seed=132, max_iterations=200)),
    # D. the float32 range
    "scale_1": (lambda: scale_base(), scale_prm(0)),
    "denormal_cloud": (lambda: denormal_case(), scale_prm(-140)),
    "threshold_1e200": (lambda: scale_base(), dict(seed=SCALE_SEED, max_iterations=SCALE_IT, inlier_threshold=1e200)),
    "threshold_2e19": (lambda: scale_base(), dict(seed=SCALE_SEED, max_iterations=SCALE_IT, inlier_threshold=2e19)),
    "threshold_1e-30": (lambda: scale_base(), dict(seed=SCALE_SEED, max_iterations=SCALE_IT, inlier_threshold=1e-30)),
    "threshold_1e-200": (lambda: scale_base(), dict(seed=SCALE_SEED, max_iterations=SCALE_IT, inlier_threshold=1e-200)),
    # min_sample_distance at 2^62, where the squared distance between two source points is a float up to 4 * 2^62 apart and +inf
    # beyond (+inf is above the square of ANY finite distance); and one whose own square is +inf in double (no two points are so far apart)
    "min_sample_distance_inf_d2": (lambda: scaled_case(62), dict(scale_prm(62), min_sample_distance=math.ldexp(2.5, 62), seed=72)),
    "min_sample_distance_1e200": (lambda: scaled_case(62), dict(min_sample_distance=1e200, **scale_prm(62))),
}
for _e in SCALE_EXPONENTS:
    CASES["scale_2^%+d" % _e] = (functools.partial(scaled_case, _e), scale_prm(_e))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(sac_ref.sac's result, source xyz, target xyz, corr, true, parameters) of a case, computed once a process"""
    from rsreg_amd import api
    make, prm = CASES[name]
    src, tgt, corr, true = make()
    return R.sac(api, src, tgt, corr, **prm), src, tgt, corr, true, prm


def capacities(n_inliers):
    return (0, 1, n_inliers - 1, n_inliers, n_inliers + 1)
