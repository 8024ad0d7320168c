"""Cases of rsreg_cloud_score_transforms and rsreg_cloud_prerejective (tests/test_prerej_cpu.py, tests/test_prerej_gpu.py), at the
smallest sizes that reach each branch: the seams of the sum tree, targets of one point and of a 4001 x 2 x 2-cell sliver, ranges from
0 to one whose square is +inf, records and transforms that are not finite, one hypothesis more than a batch.  Nothing exceeds a few
hundred points on either side and 512 hypotheses, so the brute-force reference of a case takes a second on the CPU.
"""
import collections
import functools

import numpy as np

import pointgrid_cases as G
import sac_cases as K

# csrc/prerej_plan.hpp (tests/test_prerej_cpu.py compares them with the compiled header)
BLOCK, TILE, CHUNK, MAX_GROUPS, MAX_BATCH, ROUND, PARTIAL_BYTES, PARTIAL_STRIDE = 128, 128, 16, 1 << 20, 256, 16384, 32 << 20, 16

TURN = K.rigid((0.3, -0.5, 0.8), 2.0 * np.pi / 3.0, (0.3, -0.24, 0.32))   # 120 degrees and 0.5 m
SOURCE_SIZES = (1, 3, 63, 64, 65, 127, 128, 129, 300)
STRIDES = (12, 16, 32, 48)
RANGE = 0.05


def plan(n, H):
    """(tiles, chunks, slice_chunks, slices) of csrc/prerej_plan.hpp"""
    tiles, chunks = -(-n // TILE), -(-H // CHUNK)
    per = min(max(1, -(-(tiles * chunks) // MAX_GROUPS)), chunks)
    return tiles, chunks, per, -(-chunks // per)


def batch_cap(n):
    return max(1, min(MAX_BATCH, PARTIAL_BYTES // (-(-n // TILE) * PARTIAL_STRIDE)))


def box(n, seed):
    """n points in the unit box"""
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


def moved(M, xyz):
    """M applied in float64, rounded to float32"""
    return (np.asarray(xyz, np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def base_pair():
    """(source 300, target 300): the target is TURN of the source, shuffled; every third record off by up to 0.1, so that under TURN
    about two thirds of the records are inliers at RANGE and the rest spread around it"""
    rng = np.random.default_rng(5)
    src = box(300, 1)
    tgt = moved(TURN, src)
    off = np.arange(300) % 3 == 0
    tgt[off] += (rng.normal(0, 0.04, (int(off.sum()), 3))).astype(np.float32)
    return src, tgt[rng.permutation(300)]


def transforms(H=12, seed=0):
    """(H, 4, 4) float32.  The first twelve: the identity, TURN, TURN disturbed five times, two that throw the source 2^20 m away,
    one that holds +inf, one that holds NaN, one all zero; behind them TURN disturbed at random."""
    rng = np.random.default_rng(40 + seed)
    out = np.zeros((max(H, 12), 4, 4), np.float32)
    out[:] = TURN.astype(np.float32)
    out[0] = np.eye(4)
    for j in list(range(2, 7)) + list(range(12, len(out))):
        axis = rng.normal(size=3)
        out[j] = (K.rigid(axis, rng.uniform(0, 0.05), rng.uniform(-0.03, 0.03, 3)) @ TURN).astype(np.float32)
    out[7, :3, 3] += np.float32(2.0 ** 20)
    out[8, 0, 3] = -np.float32(2.0 ** 20)
    out[9, 1, 3] = np.inf
    out[10, 2, 1] = np.nan
    out[11] = 0.0
    return out[:H]


def sliver():
    """1 500 points along x whose fitness grid is 4001 x 2 x 2 cells (pointgrid_cases: line_x)"""
    return np.array(G.scene("line_x"), np.float32)


def _score_cases():
    src, tgt = base_pair()
    c = collections.OrderedDict()
    Ts = transforms()
    for n in SOURCE_SIZES:
        c["source_%d" % n] = (src[:n], tgt, Ts, RANGE)
    c["target_one_point"] = (src[:129], tgt[:1], Ts, 0.6)
    c["target_two_coincident"] = (src[:129], np.repeat(tgt[:1], 2, axis=0), Ts, 0.6)
    line = sliver()
    rng = np.random.default_rng(9)
    near = line[rng.choice(len(line), 150, replace=False)] + rng.normal(0, 2e-4, (150, 3)).astype(np.float32)
    eye_and_far = np.stack([np.eye(4, dtype=np.float32)] * 3)
    eye_and_far[1, 0, 3], eye_and_far[2, 1, 3] = 1e-4, 2.0 ** 20
    c["target_sliver"] = (near.astype(np.float32), line, eye_and_far, 5e-4)
    c["range_zero"] = (src, tgt, Ts, 0.0)
    c["range_below_spacing"] = (src, tgt, Ts, 1e-4)
    c["range_above_box"] = (src, tgt, Ts, 10.0)
    c["range_square_inf"] = (src, tgt, Ts, 1e200)
    c["range_square_tiny"] = (tgt[:100], tgt, Ts[:2], 1e-30)            # (the square is below 2^-149: only d2 == 0 counts)
    s2, t2 = src.copy(), tgt.copy()
    s2[[0, 63, 64, 128, 299]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3, [np.inf] * 3]
    t2[[1, 100, 200]] = [[np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, np.nan]]
    c["nonfinite_records"] = (s2, t2, Ts, RANGE)
    c["nonfinite_target_only"] = (src[:65], np.full((5, 3), np.nan, np.float32), Ts[:3], RANGE)
    c["hypotheses_none"] = (src[:129], tgt, Ts[:0], RANGE)
    c["hypotheses_one"] = (src[:129], tgt, Ts[1:2], RANGE)
    c["hypotheses_past_a_batch"] = (src[:129], tgt, transforms(MAX_BATCH + 1, 3), RANGE)
    return c


SCORE_CASES = _score_cases()


# ---- the full call
def table(n_src, n_tgt, k, true_of, share, seed, minus=()):
    """(n_src, k) int32: random target records; a `share` of the rows hold true_of[row] in a random column; the rows `minus` are -1"""
    rng = np.random.default_rng(seed)
    nbr = rng.integers(0, n_tgt, (n_src, k)).astype(np.int32)
    hit = rng.random(n_src) < share
    nbr[hit, rng.integers(0, k, int(hit.sum()))] = np.asarray(true_of, np.int32)[hit]
    nbr[list(minus)] = -1
    return nbr


@functools.lru_cache(maxsize=None)
def pair(n=120, seed=3, noise=0.0):
    """(source, target, true_of): the target is TURN of the source (+ noise), shuffled; target record true_of[i] is source record i's"""
    rng = np.random.default_rng(seed)
    src = box(n, seed)
    perm = rng.permutation(n)
    tgt = np.empty_like(src)
    tgt[perm] = moved(TURN, src) + rng.normal(0, noise, (n, 3)).astype(np.float32) if noise else moved(TURN, src)
    return src, tgt, perm.astype(np.int32)


def dyadic_pair(n=60, seed=8):
    """a source on a grid of 2^-10 and its copy shifted by dyadic numbers: every edge length is EXACTLY equal on both sides"""
    rng = np.random.default_rng(seed)
    src = (rng.integers(0, 1024, (n, 3)) / 1024.0).astype(np.float32)
    tgt = (src + np.float32([0.5, 0.25, -1.0])).astype(np.float32)
    return src, tgt, np.arange(n, dtype=np.int32)


def decoy_case():
    """Twelve source records.  The target holds their TURNed copies with noise of 1e-3, and EXACT copies of records 0 .. 5 under
    another motion.  k = 1: rows 0 .. 5 name the exact copies, rows 6 .. 11 the noisy ones.  A sample inside 0 .. 5 gives a pose
    with six inliers at an error of rounding; one inside 6 .. 11 gives twelve inliers at the noise's error.  PCL's rule takes the
    first kind, select_by_inliers the second."""
    rng = np.random.default_rng(21)
    src = box(12, 21)
    other = K.rigid((0.9, 0.1, -0.2), 1.0, (3.0, 3.0, 3.0))
    tgt = np.concatenate([moved(TURN, src) + rng.normal(0, 1e-3, (12, 3)).astype(np.float32), moved(other, src[:6])]).astype(np.float32)
    nbr = np.concatenate([12 + np.arange(6), 6 + np.arange(6)]).astype(np.int32).reshape(12, 1)
    return src, tgt, nbr, dict(max_iterations=512, max_correspondence_distance=RANGE, seed=2)


def _prerej_cases():
    c = collections.OrderedDict()
    src, tgt, true_of = pair()
    n = len(src)
    for k, sim in ((1, 0.9), (2, 0.9), (5, 0.8), (16, 0.5)):
        c["k_%d" % k] = (src, tgt, table(n, n, k, true_of, 0.7, 10 + k, minus=(0, 7, 64, n - 1)),
                         dict(max_iterations=192, similarity_threshold=sim, max_correspondence_distance=RANGE, seed=k))
    c["all_ineligible"] = (src, tgt, np.full((n, 2), -1, np.int32), dict(max_iterations=64, max_correspondence_distance=RANGE))
    c["polygon_always_fails"] = (src, (tgt * np.float32(10.0)).astype(np.float32), table(n, n, 2, true_of, 0.7, 31),
                                 dict(max_iterations=128, max_correspondence_distance=RANGE))
    c["similarity_zero"] = (src, tgt, table(n, n, 2, true_of, 0.3, 32), dict(max_iterations=64, similarity_threshold=0.0, max_correspondence_distance=RANGE, seed=5))
    ds, dt, dtrue = dyadic_pair()
    c["similarity_just_under_one"] = (ds, dt, table(len(ds), len(dt), 1, dtrue, 0.8, 33),
                                      dict(max_iterations=128, similarity_threshold=float(np.nextafter(np.float32(1), np.float32(0))),
                                           max_correspondence_distance=RANGE, seed=6))
    nsrc, ntgt, ntrue = pair(120, 4, 0.01)
    noisy = table(len(nsrc), len(ntgt), 1, ntrue, 0.7, 34)
    for name, frac in (("fraction_0", 0.0), ("fraction_half", 0.5), ("fraction_1", 1.0)):
        c[name] = (nsrc, ntgt, noisy, dict(max_iterations=192, max_correspondence_distance=0.02, inlier_fraction=frac, seed=7))
    d = decoy_case()
    c["decoy_pcl_rule"] = (d[0], d[1], d[2], dict(d[3], select_by_inliers=0))
    c["decoy_by_inliers"] = (d[0], d[1], d[2], dict(d[3], select_by_inliers=1))
    one = table(n, n, 1, true_of, 0.7, 35)
    c["iterations_0"] = (src, tgt, one, dict(max_iterations=0, max_correspondence_distance=RANGE))
    c["iterations_1"] = (src, tgt, one, dict(max_iterations=1, max_correspondence_distance=RANGE, seed=3))
    c["seed_0"] = (src, tgt, one, dict(max_iterations=128, max_correspondence_distance=RANGE, seed=0))
    c["seed_2_63"] = (src, tgt, one, dict(max_iterations=128, max_correspondence_distance=RANGE, seed=1 << 63))
    c["past_a_batch"] = (src, tgt, one, dict(max_iterations=MAX_BATCH + 1, max_correspondence_distance=RANGE, seed=9, select_by_inliers=1))
    s2, t2 = src.copy(), tgt.copy()
    s2[[3, 50]] = [[np.nan, 0, 0], [0, np.inf, 0]]
    t2[true_of[[10, 20]]] = [[np.nan] * 3, [0, -np.inf, 0]]
    c["nonfinite_records"] = (s2, t2, one, dict(max_iterations=192, max_correspondence_distance=RANGE, seed=4))
    c["default_range"] = (src[:40], tgt, table(40, n, 1, true_of[:40], 0.9, 36), dict(max_iterations=32, seed=1))   # sqrt(DBL_MAX): its square is above FLT_MAX
    return c


PREREJ_CASES = _prerej_cases()


@functools.lru_cache(maxsize=None)
def end_to_end():
    """400 points in the unit box and their copy under TURN; 40 % of the rows hold the true match among k = 5, the rest are random;
    range 0.05, 512 iterations, select_by_inliers.  The seed is the first for which the reference finds every source record an
    inlier (tests/test_prerej_cpu.py checks that it does)."""
    src, tgt, true_of = pair(400, 12)
    nbr = table(400, 400, 5, true_of, 0.4, 50)
    return src, tgt, nbr, dict(max_iterations=512, max_correspondence_distance=0.05, select_by_inliers=1, seed=END_TO_END_SEED)


END_TO_END_SEED = 1
