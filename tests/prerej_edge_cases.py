"""The cases of tests/test_prerej_edges_cpu.py and tests/test_prerej_edges_gpu.py: what tests/prerej_cases.py does not reach.  Second
and later rounds of hypotheses (a winner in the second round, a last round of one hypothesis, transforms scored past a round), a source
of 8 193 tiles, whose batch is capped below prerej_cases.MAX_BATCH, degenerate samples (sources of 1 .. 4 records, exact ties,
collinear and coincident sources, one target record, a mirrored target, one cloud on both sides), and the float32 range (both clouds
times 2^e, a cloud of denormals, a range AT a float d2, a cloud at 2^62 under transforms that hold FLT_MAX and denormals).

What each case is FOR is asserted on the reference by tests/test_prerej_edges_cpu.py; the GPU test compares bits.  Every cloud comes
from a fixed seed; where a seed was picked, the condition it was picked for is stated here and asserted there.
"""
import collections
import functools
import math

import numpy as np

import prerej_cases as C
import prerej_ref as R
import sac_edge_cases as E

ROUND = C.ROUND
FLT_MIN = np.float32(np.finfo(np.float32).tiny)
JUST_UNDER_ONE = float(np.nextafter(np.float32(1), np.float32(0)))


def true_table(true_of):
    return np.asarray(true_of, np.int32).reshape(-1, 1).copy()


# ---- A. rounds and batches
# the seeds of rounds_full_call: with the first the reference's winner lies in the SECOND round (hypothesis 29 456; 47 + 59 valid),
# with the second in the first (hypothesis 862; 60 + 49 valid).  One reference takes 1.5 s on the CPU.
ROUNDS_SEED_LATE, ROUNDS_SEED_EARLY = 6, 5


def rounds_case(seed, select_by_inliers=0):
    """40 records with noise of 0.005; three rows in four of the table are ineligible, so that most hypotheses end after their draws
    and a round of 16 384 holds some 50 valid ones; 2 * ROUND + 1 hypotheses: three rounds, the last of one hypothesis"""
    src, tgt, true_of = C.pair(40, 6, 0.005)
    nbr = C.table(40, 40, 1, true_of, 0.8, 60, minus=[i for i in range(40) if i % 4 != 0])
    return src, tgt, nbr, dict(max_iterations=2 * ROUND + 1, max_correspondence_distance=0.03, seed=seed, select_by_inliers=select_by_inliers)


PAST_ROUND_H, PAST_ROUND_SEED = ROUND + 17, 0


def score_past_a_round():
    """(source 129, target 300, the 12 distinct transforms, which of them each of the ROUND + 17 rows is, the range).  The seed of
    the pick is the first for which rows ROUND - 1, ROUND and ROUND + 16 are three different transforms of which two have different
    non-zero counts."""
    src, tgt = C.base_pair()
    return src[:129], tgt, C.transforms(), np.random.default_rng(PAST_ROUND_SEED).integers(0, 12, PAST_ROUND_H), C.RANGE


CAP_N, CAP_H, CAP_RANGE, CAP_SEED = C.TILE * 8193, 256, 1.0, 38
CAP_NAN = 3                                                       # which of the four distinct transforms holds the NaN


@functools.lru_cache(maxsize=None)
def batch_cap_below_256():
    """(source of 128 * 8193 records, target of 5, the 4 distinct transforms, which of them each of the 256 rows is, the range).
    8 193 tiles: prerej_cases.batch_cap gives 255, so 256 rows go out as a batch of 255 and a batch of 1, and the partial sums of a
    hypothesis lie 8 193 groups apart.  The source is the unit box moved by TURN, with noise of 0.02; the target five points of the box
    moved by TURN; the transforms TURN, two disturbed TURNs and one that holds a NaN.  The seed of the pick is the first for which
    rows 0, 254 and 255 are three different transforms, none of them the NaN one.
    The reference of the 4 distinct transforms takes 1.1 s on the CPU (measured: one core, numpy), under the 5 s at which the
    distinct transforms would be cut to 3."""
    rng = np.random.default_rng(70)
    src = (C.moved(C.TURN, C.box(CAP_N, 70)) + rng.normal(0, 0.02, (CAP_N, 3)).astype(np.float32)).astype(np.float32)
    tgt = C.moved(C.TURN, C.box(5, 71))
    return src, tgt, C.transforms()[[1, 2, 3, 10]], np.random.default_rng(CAP_SEED).integers(0, 4, CAP_H), CAP_RANGE


# ---- B. degenerate samples
def line_case():
    """60 points of sac_edge_cases.line(), exactly collinear, and the line turned by 90 degrees about z and shifted by integers:
    both exact in float32, every edge has the same squared length on both sides.  Observed on the reference: the host solve
    completes the rank-1 sample, n_valid = 120 of 128 (every hypothesis of three distinct records), 60 inliers"""
    src = E.line(60, seed=45)
    tgt = np.stack([-src[:, 1] + 3, src[:, 0] - 2, src[:, 2] + 1], axis=1).astype(np.float32)
    return src, tgt


def twins():
    """40 records, 2i and 2i + 1 the same point, and their TURN image"""
    src = np.repeat(C.box(20, 46), 2, axis=0)
    return src, C.moved(C.TURN, src)


def mirrored():
    """60 points of the unit box and their reflection in z = 0 (exact)"""
    src = C.box(60, 47)
    return src, (src * np.float32([1, 1, -1])).astype(np.float32)


def scaled_pair(e):
    src, tgt, true_of = C.pair(60, 3)
    return E.scaled(src, e), E.scaled(tgt, e), true_of


def denormal_pair():
    """sac_edge_cases.denormal_case's recipe on pair(60, 3): moved to positive coordinates, at 2^-140"""
    src, tgt, true_of = C.pair(60, 3)
    return E.scaled(src + np.float32(3.0), -140), E.scaled(tgt + np.float32(7.0), -140), true_of


SCALE_EXPONENTS = E.SCALE_EXPONENTS
SAME_CLOUD = ("same_cloud",)                                      # the cases whose source and target are ONE device cloud


def _cases():
    c = collections.OrderedDict()
    c["rounds_winner_in_round_2"] = rounds_case(ROUNDS_SEED_LATE)
    c["rounds_winner_in_round_1"] = rounds_case(ROUNDS_SEED_EARLY)
    c["rounds_by_inliers"] = rounds_case(ROUNDS_SEED_LATE, 1)
    for n in (1, 2, 3, 4):
        src, tgt, true_of = C.pair(n, 9)
        c["ns_%d" % n] = (src, tgt, true_table(true_of), dict(max_iterations=128, max_correspondence_distance=C.RANGE, seed=2))
    src, tgt, true_of = C.pair(4, 7)
    for rule in (0, 1):
        c["ties_first_wins_rule_%d" % rule] = (src, tgt, true_table(true_of), dict(max_iterations=128, max_correspondence_distance=C.RANGE, seed=3, select_by_inliers=rule))
    src, tgt = line_case()
    c["collinear_sources"] = (src, tgt, true_table(np.arange(60)), dict(max_iterations=128, similarity_threshold=JUST_UNDER_ONE, max_correspondence_distance=C.RANGE, seed=4))
    src, tgt = twins()
    for sim in (0.9, 0.0):
        c["coincident_sources_sim_%g" % sim] = (src, tgt, true_table(np.arange(40)), dict(max_iterations=128, similarity_threshold=sim, max_correspondence_distance=C.RANGE, seed=5))
    # every row names target record 7.  Observed on the reference: at 0.9 nothing is valid; at 0 every edge is 0 / ds = 0 >= 0, the
    # rank-0 solve succeeds on all 123 hypotheses of three distinct records, and the winner has one inlier
    src, tgt, true_of = C.pair(60, 10)
    for sim in (0.0, 0.9):
        c["one_target_record_sim_%g" % sim] = (src, tgt, np.full((60, 1), 7, np.int32), dict(max_iterations=128, similarity_threshold=sim, max_correspondence_distance=C.RANGE, seed=6))
    src, tgt = mirrored()
    c["mirrored_target"] = (src, tgt, true_table(np.arange(60)), dict(max_iterations=128, max_correspondence_distance=C.RANGE, seed=7))
    src = C.box(60, 48)
    c["same_cloud"] = (src, src, C.table(60, 60, 1, np.arange(60), 0.7, 61), dict(max_iterations=128, max_correspondence_distance=C.RANGE, seed=8))
    for e in SCALE_EXPONENTS:
        src, tgt, true_of = scaled_pair(e)
        prm = dict(max_iterations=64, max_correspondence_distance=math.ldexp(0.05, e), seed=1)
        c["scale_2^%+d" % e] = (src, tgt, true_table(true_of), prm)
        if e in (-70, 62):                                       # 30 % random rows: the division also decides edges that fail
            c["scale_2^%+d_random_rows" % e] = (src, tgt, C.table(60, 60, 1, true_of, 0.7, 62), prm)
        if e == 62:                                              # ... and at threshold 0 wrong samples are valid: their poses throw source records out of the float range
            c["scale_2^+62_random_rows_sim_0"] = (src, tgt, C.table(60, 60, 1, true_of, 0.7, 62), dict(prm, similarity_threshold=0.0))
    src, tgt, true_of = denormal_pair()
    c["denormal_cloud"] = (src, tgt, true_table(true_of), dict(max_iterations=64, max_correspondence_distance=math.ldexp(0.05, -140), seed=1))
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    """prerej_ref.prerejective's result of a case, computed once a process"""
    from rsreg_amd import api
    src, tgt, nbr, prm = CASES[name]
    return R.prerejective(api, src, tgt, nbr, **prm)


@functools.lru_cache(maxsize=None)
def edges(name):
    """{h: prerej_ref.sample_edges} of the hypotheses of a case that reach the polygon test"""
    src, tgt, nbr, prm = CASES[name]
    out = {}
    for h in range(prm["max_iterations"]):
        e = R.sample_edges(R.xyz_of(src), R.xyz_of(tgt), nbr, prm["seed"], h)
        if e is not None:
            out[h] = e
    return out


@functools.lru_cache(maxsize=None)
def distinct_scores(which):
    """(counts, sums) of the DISTINCT transforms of score_past_a_round / batch_cap_below_256: the rows' scores are these, indexed by the pick"""
    src, tgt, Ts, pick, rng = score_past_a_round() if which == "past_a_round" else batch_cap_below_256()
    return R.score_transforms(Ts, src, tgt, rng)


# ---- C. a range AT a float d2: one source record, one or two target records, the identity
def range_pairs():
    """[(label, source (1, 3), target (1 or 2, 3), d2 float32)]: d2 is 0, 2^-149, 2^-148, 0.0625, 0.875, the largest float below
    2^127, +inf by overflow.  The differences are dyadic numbers of a few bits, so that every square and sum is exact and d2 is what
    the label says (asserted by the CPU test); where there are two target records the second is farther away."""
    root = np.float32(np.sqrt(2.0) * 2.0 ** -75)                  # root * root = 2^-149 (1 - 2e-8), which rounds to 2^-149
    far = np.float32([-3.0, 2.0, 1.0])
    rows = [("0", [3.0, -2.0, 0.5], [[3.0, -2.0, 0.5], far]),
            ("2^-149", [0, 0, 0], [[root, 0, 0]]),
            ("2^-148", [0, 0, 0], [[2.0 ** -74, 0, 0]]),
            ("0.0625", [0, 0, 0], [[0.25, 0, 0], far]),
            ("0.875", [1.0, 1.0, 1.0], [[1.75, 0.5, 1.25]]),
            ("below 2^127", [0, 0, 0], [BIG_D_XYZ]),
            ("+inf", [0, 0, 0], [[2.0 ** 64, 0, 0]])]
    out = []
    for label, s, t in rows:
        s, t = np.float32([s]), np.float32(t)
        out.append((label, s, t, R.nearest_d2(s, t)[0]))
    return out


# 2^127 (1 - 2^-24) = 2^103 (2^24 - 1) = 2^102 (a^2 + b^2 + c^2): each square and the sum of the first two are floats
BIG_D_ABC = (4093, 1609, 3770)
BIG_D_XYZ = [math.ldexp(v, 51) for v in BIG_D_ABC]
FIXED_RANGES = (0.0, 1e-200, 1e-30, 2e19, 1e200)


def ranges_around(d2):
    """(ranges whose double square is <= d2, ranges whose square is > d2) next to sqrt(d2), d2 a finite float: the largest double r
    with r * r <= d2 and the one below it; the one above it.  Where sqrt(d2) is exact in double the first IS sqrt(d2).
    d2 == 0: the ranges 0 and the least double above it, whose square is 0 as well: by the contract's rule ((double)d2 < range * range,
    the product a double) neither makes the record an inlier; the least range that does is the first whose square is not 0."""
    d2 = float(d2)
    if d2 == 0.0:
        r = math.ldexp(math.sqrt(2.0), -538)                      # 2^-537.5: its square is half the least double, a tie
        for _ in range(8):
            if r * r > 0.0 and float(np.nextafter(r, 0.0)) ** 2 > 0.0:
                r = float(np.nextafter(r, 0.0))
            elif r * r == 0.0:
                r = float(np.nextafter(r, math.inf))
        assert r * r > 0.0 and float(np.nextafter(r, 0.0)) ** 2 == 0.0
        return [0.0, 5e-324, float(np.nextafter(r, 0.0))], [r]
    r = math.sqrt(d2)
    while r * r > d2:
        r = float(np.nextafter(r, 0.0))
    while float(np.nextafter(r, math.inf)) ** 2 <= d2:
        r = float(np.nextafter(r, math.inf))
    out = [r] if r == 0.0 else [r, float(np.nextafter(r, 0.0))]
    return out, [float(np.nextafter(r, math.inf))]


# ---- C. a cloud at 2^62 under transforms that throw it out of the float range
THROWN_RANGES = (2.0 ** 62, 1e200)                                # the cloud's own scale; a square of +inf: a record counts iff its d2 is finite


def thrown_out_of_range():
    """(source, target, the 14 transforms of sac_edge_cases.extreme_transforms_case): pair(60, 3) at 2^62"""
    src, tgt, _ = scaled_pair(62)
    return src, tgt, E.extreme_transforms_case()[3]
