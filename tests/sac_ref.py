"""The numpy reference of the pose-from-correspondences contract (include/rsreg.h): the counter-based generator in numpy.uint64, a
hypothesis's three-pair sums in float64 in the contract's order with the solve through api.umeyama_from_sums (the host solve,
which is not code under test), the scores in numpy.float32 in the contract's order, and the stopping rule replayed with math.log.

Nothing here knows about batches, tiles or slices: a hypothesis is a function of (seed, h), a count a function of (T, pairs).
Trace (at the end) runs the float32 operations once more and classifies every intermediate: tests/test_sac_edges_cpu.py reads from it
in which regime of the float32 range a scaled case lies.
"""
import math

import numpy as np

M64 = (1 << 64) - 1
GOLDEN, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
TRIES = 16
NUM_SUMS = 17
EPS = float(np.finfo(np.float64).eps)


def draw_index(seed, h, draw, n):
    """index(h, draw) of the contract, every step in numpy.uint64 (which wraps modulo 2^64); h and draw may be arrays"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.uint64(64) * np.asarray(h, np.uint64) + np.asarray(draw, np.uint64)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        z = z ^ (z >> np.uint64(31))
        return ((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)


def pair_points(src_xyz, tgt_xyz, corr):
    """(P, Q, finite): the float32 source and target point of every pair and whether all six coordinates are finite"""
    P = np.ascontiguousarray(src_xyz, np.float32)[corr["index_query"]].reshape(-1, 3)
    Q = np.ascontiguousarray(tgt_xyz, np.float32)[corr["index_match"]].reshape(-1, 3)
    return P, Q, np.isfinite(P).all(axis=1) & np.isfinite(Q).all(axis=1)


def l2_simple(a, b):
    """float32 (dx * dx + dy * dy) + dz * dz, every operation rounded once"""
    with np.errstate(all="ignore"):
        d = (a.astype(np.float32) - b.astype(np.float32)).astype(np.float32)
        return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)


def three_pair_sums(P, Q, ids):
    """the 17 sums of the pairs ids[0], ids[1], ids[2] in float64, each 0.0 + the three terms in pair order"""
    s = np.zeros(NUM_SUMS, np.float64)
    for i in ids:
        p, q = P[i].astype(np.float64), Q[i].astype(np.float64)
        s[0] += 1.0
        s[1:4] += p
        s[4:7] += q
        s[7:16] += np.outer(q, p).ravel()
        s[16] += np.float64(l2_simple(P[i], Q[i]))
    return s


def hypothesis(api, P, Q, finite, seed, h, min_sample_distance=0.0):
    """(T 4 x 4 float32 or None, (i0, i1, i2) or None, the try): hypothesis h of the contract"""
    n = len(P)
    msd2 = float(min_sample_distance) * float(min_sample_distance)
    for t in range(TRIES):
        ids = [int(draw_index(seed, h, 3 * t + k, n)) for k in range(3)]
        if len(set(ids)) < 3 or not finite[ids].all():
            continue
        if not all(float(l2_simple(P[ids[a]], P[ids[b]])) > msd2 for a, b in ((0, 1), (0, 2), (1, 2))):
            continue
        return api.umeyama_from_sums(three_pair_sums(P, Q, ids)), tuple(ids), t
    return None, None, -1


def hypotheses(api, P, Q, finite, seed, H, min_sample_distance=0.0, first=0):
    """[(T or None, ids or None)] of the hypotheses first .. first + H - 1"""
    return [hypothesis(api, P, Q, finite, seed, first + j, min_sample_distance)[:2] for j in range(H)]


def within(T, P, Q, finite, threshold):
    """bool per pair (or per (transform, pair) when T is (H, 4, 4)): inlier under T, the contract's float32 score"""
    T = np.asarray(T, np.float32)
    lead = T.shape[:-2]
    m = T.reshape(-1, 4, 4)[:, :3, :]
    x, y, z = P[None, :, 0], P[None, :, 1], P[None, :, 2]
    with np.errstate(all="ignore"):
        out = []
        for r in range(3):
            a = (m[:, r, 0, None] * x).astype(np.float32) + (m[:, r, 1, None] * y).astype(np.float32)
            a = a.astype(np.float32) + (m[:, r, 2, None] * z).astype(np.float32)
            out.append((a.astype(np.float32) + m[:, r, 3, None]).astype(np.float32))
        dx, dy, dz = out[0] - Q[None, :, 0], out[1] - Q[None, :, 1], out[2] - Q[None, :, 2]
        d2 = ((dx * dx + dy * dy).astype(np.float32) + dz * dz).astype(np.float32)
        assert d2.dtype == np.float32
        ok = (d2.astype(np.float64) < float(threshold) * float(threshold)) & finite[None, :]
    return ok.reshape(lead + (len(P),))


def count_inliers(Ts, P, Q, finite, threshold, chunk=512):
    Ts = np.asarray(Ts, np.float32).reshape(-1, 4, 4)
    out = np.zeros(len(Ts), np.uint32)
    for a in range(0, len(Ts), chunk):
        out[a:a + chunk] = within(Ts[a:a + chunk], P, Q, finite, threshold).sum(axis=1)
    return out


def replay(counts, n, probability, max_iterations, check_margin=True, valid=None):
    """(best, winner, iterations, ks): PCL's stopping rule over counts[0 ..] in hypothesis order (valid: which hypotheses found a
    good try; None: all).  best starts at -1, PCL's -INT_MAX: the first valid hypothesis always sets k.  counts may be longer than what
    the rule consumes; IndexError if it is shorter.  check_margin: every k computed stays at least 1e-9 * k away from an integer,
    so that a log that differs in its last bits cannot change how many hypotheses are consumed (a condition on the CASE)."""
    k, best, winner, h, ks = 1.0, -1, -1, 0, []
    log_probability = math.log(1.0 - probability)
    while h < k and h < max_iterations:
        if (valid is None or valid[h]) and counts[h] > best:
            best, winner = int(counts[h]), h
            w = float(best) / float(n)
            q = 1.0 - w * w * w
            q = min(max(q, EPS), 1.0 - EPS)
            k = log_probability / math.log(q)
            ks.append(k)
            if check_margin and k <= max_iterations + 1:   # (a larger k never decides anything: h < max_iterations does)
                assert abs(k - round(k)) >= 1e-9 * k, ("the case puts k within 1e-9 of an integer: pick another seed", k)
        h += 1
    return best, winner, h, ks


class Sac:
    """What rsreg_cloud_sac_correspondences returns, from the reference"""


def sac(api, src_xyz, tgt_xyz, corr, inlier_threshold=0.05, max_iterations=1000, probability=0.99, refit_rounds=0, min_sample_distance=0.0, seed=0,
        counts=None, fit=None):
    """The rejector.  `counts` (optional): the counts of hypotheses 0 .. max_iterations - 1 computed before (they do not depend on
    the stopping rule), as (counts, valid).  `fit` (refit_rounds > 0): fit(flags) -> (T, sums) of TransformationEstimationSVD over the flagged pairs."""
    r = Sac()
    n = len(corr)
    P, Q, finite = pair_points(src_xyz, tgt_xyz, corr)
    r.transform, r.found, r.best_hypothesis, r.sample, r.iterations, r.n_inliers = np.eye(4, dtype=np.float32), False, -1, (-1, -1, -1), 0, 0
    r.refit_rounds_run, r.sums, r.kept, r.ks = 0, np.zeros(NUM_SUMS), corr.copy(), []
    if n < 3:
        return r
    if counts is None:
        hyp = hypotheses(api, P, Q, finite, seed, max_iterations, min_sample_distance)
        valid = np.array([t is not None for t, _ in hyp])
        nan = np.full((4, 4), np.nan, np.float32)
        counts = count_inliers(np.array([nan if t is None else t for t, _ in hyp]).reshape(-1, 4, 4), P, Q, finite, inlier_threshold)
    else:
        counts, valid = counts
    best, winner, r.iterations, r.ks = replay(counts, n, probability, max_iterations, valid=valid)
    r.counts, r.valid, r.best = counts, valid, best
    if best < 3:
        return r
    T, ids, _ = hypothesis(api, P, Q, finite, seed, winner, min_sample_distance)
    flags = within(T, P, Q, finite, inlier_threshold)
    assert flags.sum() == best
    r.found, r.best_hypothesis, r.sample = True, winner, ids
    for _ in range(refit_rounds):
        if flags.sum() < 3:
            break
        T, r.sums = fit(flags)
        r.refit_rounds_run += 1
        again = within(T, P, Q, finite, inlier_threshold)
        same = (again == flags).all()
        flags = again
        if same:
            break
    r.transform, r.n_inliers, r.kept, r.flags = T, int(flags.sum()), corr[flags], flags
    return r


def sum_tree_depth(n):
    """m of the bound m * 2^-53 * sum|terms| on each of the 17 sums of rsreg_cloud_estimate_rigid_svd over n pairs: the most
    additions any one term passes through in the order the contract writes out.  A term enters its wave's tree as a leaf: 6
    pairwise steps (lane bits 5 .. 0); 1 addition joins the two waves of a group of 128; a strand adds the groups g, g + 256, ..
    one after the other, ceil(groups / 256) additions at most (the first onto 0.0); 6 steps fold a 64's strands; 3 additions join
    the four 64s.  Each addition rounds once (relative error <= 2^-53) and the partial sums are bounded by sum|terms|, so to first
    order the error is at most depth * 2^-53 * sum|terms| (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., §4.2: any
    order of recursive summation, with the tree's height in the place of n - 1).  The products of two floats have 48 significant
    bits and are exact in float64, so the terms themselves carry no error."""
    groups = -(-n // 128)
    return 6 + 1 + -(-groups // 256) + 6 + 3


def exact_terms(P, Q, finite):
    """(17, n) float64: the terms of the 17 sums, exact (zeros for a pair that is not finite)"""
    n = len(P)
    t = np.zeros((NUM_SUMS, n), np.float64)
    p, q = P.astype(np.float64), Q.astype(np.float64)
    t[0] = 1.0
    t[1:4] = p.T
    t[4:7] = q.T
    for r in range(3):
        for c in range(3):
            t[7 + 3 * r + c] = q[:, r] * p[:, c]
    t[16] = l2_simple(P, Q).astype(np.float64)
    t[:, ~finite] = 0.0
    return t


class Trace:
    """The float32 operations of the contract once more, with every result classified: `inf` counts the results that overflowed
    (+-inf from finite operands), `nan` the NaNs, `denormal` the results that are non-zero denormals, `underflow` the products that
    are 0 although neither factor is.  (A float32 sum or difference cannot underflow: a denormal result of an addition is exact.)
    A run in which all four stay 0 commutes with a scaling of every input by a power of two."""
    FLT_MIN = np.float32(np.finfo(np.float32).tiny)

    def __init__(self):
        self.inf = self.nan = self.denormal = self.underflow = 0

    def _note(self, r, a, b):
        self.inf += int((np.isinf(r) & np.isfinite(a) & np.isfinite(b)).sum())
        self.nan += int(np.isnan(r).sum())
        self.denormal += int(((r != 0) & (np.abs(r) < self.FLT_MIN)).sum())
        return r

    def mul(self, a, b):
        with np.errstate(all="ignore"):
            a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
            r = (a * b).astype(np.float32)
            self.underflow += int(((r == 0) & (a != 0) & (b != 0)).sum())
        return self._note(r, a, b)

    def add(self, a, b, sign=1):
        with np.errstate(all="ignore"):
            a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
            r = (a + b if sign > 0 else a - b).astype(np.float32)
        return self._note(r, a, b)

    def l2_simple(self, a, b):
        """l2_simple() of two (.., 3) arrays, traced"""
        d = [self.add(a[..., c], b[..., c], -1) for c in range(3)]
        return self.add(self.add(self.mul(d[0], d[0]), self.mul(d[1], d[1])), self.mul(d[2], d[2]))

    def score(self, T, P, Q):
        """the float32 d2 of every pair under ONE transform T, traced: what within() compares with the threshold"""
        m = np.asarray(T, np.float32).reshape(4, 4)
        moved = []
        for r in range(3):
            a = self.add(self.mul(m[r, 0], P[:, 0]), self.mul(m[r, 1], P[:, 1]))
            moved.append(self.add(self.add(a, self.mul(m[r, 2], P[:, 2])), m[r, 3]))
        return self.l2_simple(np.stack(moved, axis=1), Q)
