"""The numpy reference of the plane-segmentation contract (include/rsreg.h, "plane segmentation"): the generator of tests/sac_ref.py,
a hypothesis's cross product and unit normal in numpy.float32 operation by operation, the axis test in Python floats (float64, one
rounding an operation), the distances in numpy.float32 in the contract's order, the stopping rule with its skip counter replayed
with math.log, and the ten sums added in the contract's tree.

Nothing here knows about batches, tiles or slices: a hypothesis is a function of (seed, h), a count a function of (model, cloud).
"""
import math

import numpy as np

from sac_ref import EPS, TRIES, draw_index

NUM_SUMS = 10
F = np.float32
NAN4 = np.full(4, np.nan, np.float32)


def finite_records(xyz):
    return np.isfinite(np.asarray(xyz, np.float32)).all(axis=1)


def distances(coeffs, xyz):
    """float32 (H, n): ((a * x + b * y) + c * z) + d, every operation rounded once"""
    m = np.asarray(coeffs, np.float32).reshape(-1, 4)
    P = np.asarray(xyz, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        s = (m[:, 0, None] * P[None, :, 0]).astype(F) + (m[:, 1, None] * P[None, :, 1]).astype(F)
        s = s.astype(F) + (m[:, 2, None] * P[None, :, 2]).astype(F)
        s = (s.astype(F) + m[:, 3, None]).astype(F)
    assert s.dtype == np.float32
    return s


def within(coeffs, xyz, threshold):
    """bool (H, n): the record is finite and (double)|dist| < threshold, strictly"""
    d = distances(coeffs, xyz)
    with np.errstate(all="ignore"):
        return (np.abs(d).astype(np.float64) < float(threshold)) & finite_records(xyz)[None, :]


def count(coeffs, xyz, threshold, chunk=256):
    m = np.asarray(coeffs, np.float32).reshape(-1, 4)
    out = np.zeros(len(m), np.uint32)
    for a in range(0, len(m), chunk):
        out[a:a + chunk] = within(m[a:a + chunk], xyz, threshold).sum(axis=1)
    return out


def axis_on(axis, eps_angle):
    return eps_angle > 0.0 and any(float(a) != 0.0 for a in axis)


def axis_cs(coeff, axis):
    """the contract's cs in float64, every written operation rounded once"""
    a, b, c = (float(v) for v in coeff[:3])
    ax, ay, az = (float(v) for v in axis)
    return abs((a * ax + b * ay) + c * az) / (math.sqrt((a * a + b * b) + c * c) * math.sqrt((ax * ax + ay * ay) + az * az))


def hypothesis(xyz, finite, seed, h, axis=(0.0, 0.0, 0.0), eps_angle=0.0):
    """(model (4,) float32 -- NaN when invalid, sample (4,) int32, valid, cs or None): hypothesis h of the contract"""
    P = np.asarray(xyz, np.float32)
    n = len(P)
    sample, model = np.full(4, -1, np.int32), None
    with np.errstate(all="ignore"):
        for t in range(TRIES if n >= 3 else 0):
            ids = [int(draw_index(seed, h, 3 * t + k, n)) for k in range(3)]
            if len(set(ids)) < 3 or not finite[ids].all():
                continue
            p0, p1, p2 = P[ids[0]], P[ids[1]], P[ids[2]]
            u, v = (p1 - p0).astype(F), (p2 - p0).astype(F)
            nx = F(F(u[1] * v[2]) - F(u[2] * v[1]))
            ny = F(F(u[2] * v[0]) - F(u[0] * v[2]))
            nz = F(F(u[0] * v[1]) - F(u[1] * v[0]))
            n2 = F(F(F(nx * nx) + F(ny * ny)) + F(nz * nz))
            if not (np.isfinite(n2) and n2 > 0):
                continue
            l = np.sqrt(n2)
            assert l.dtype == np.float32
            a, b, c = F(nx / l), F(ny / l), F(nz / l)
            d = F(-F(F(F(a * p0[0]) + F(b * p0[1])) + F(c * p0[2])))
            model = np.array([a, b, c, d], np.float32)
            sample = np.array(ids + [t], np.int32)
            break
    if model is None:
        return NAN4.copy(), sample, False, None
    if not axis_on(axis, eps_angle):
        return model, sample, True, None
    cs = axis_cs(model, axis)
    ok = cs >= math.cos(eps_angle)
    return (model if ok else NAN4.copy()), sample, bool(ok), cs


def hypotheses(xyz, seed, first, H, axis=(0.0, 0.0, 0.0), eps_angle=0.0):
    """(models (H, 4), samples (H, 4), valid (H,), cs list) of the hypotheses first .. first + H - 1"""
    finite = finite_records(xyz)
    rows = [hypothesis(xyz, finite, seed, first + j, axis, eps_angle) for j in range(H)]
    return (np.array([r[0] for r in rows], np.float32).reshape(H, 4), np.array([r[1] for r in rows], np.int32).reshape(H, 4),
            np.array([r[2] for r in rows], bool), [r[3] for r in rows])


class Replay:
    """PCL's stopping rule with its skip counter, one hypothesis at a time.  check_margin: every k computed stays at least 1e-9 * k
    away from an integer, so that a log that differs in its last bits cannot change how many hypotheses are consumed (a condition on
    the CASE)."""

    def __init__(self, n, probability, max_iterations, check_margin=True):
        self.n, self.max_iterations, self.check_margin = n, max_iterations, check_margin
        self.log_probability = math.log(1.0 - probability)
        self.k, self.it, self.skipped, self.best, self.winner, self.next, self.ks = 1.0, 0, 0, -1, -1, 0, []

    def wants_more(self):
        return self.it < self.k and self.it < self.max_iterations and self.skipped < 10 * self.max_iterations

    def feed(self, valid, c):
        h = self.next
        self.next += 1
        if not valid:
            self.skipped += 1
            return
        if int(c) > self.best:
            self.best, self.winner = int(c), h
            w = float(self.best) / float(self.n)
            q = 1.0 - w * w * w
            q = min(max(q, EPS), 1.0 - EPS)
            self.k = self.log_probability / math.log(q)
            self.ks.append(self.k)
            if self.check_margin and self.k <= self.max_iterations + 1:
                assert abs(self.k - round(self.k)) >= 1e-9 * self.k, ("the case puts k within 1e-9 of an integer: pick another seed", self.k)
        self.it += 1


def replay(counts, valid, n, probability, max_iterations, check_margin=False):
    """(best, winner, iterations, skipped) over the given sequences; IndexError if the rule wants more than they hold"""
    r = Replay(n, probability, max_iterations, check_margin)
    while r.wants_more():
        r.feed(valid[r.next], counts[r.next])
    return r.best, r.winner, r.it, r.skipped


def tree_sum(terms):
    """the contract's fixed tree over the last axis of `terms` (.., n) float64: term i is lane i % 64 of wave (i / 64) % 2 of group
    i / 128; a wave's 64 terms meet pairwise across lane bit 5, 4, .., 0; a group is wave 0 + wave 1; groups g, g + 256, .. are added
    in ascending order onto 0.0 into one of 256 strands; strand t meets t + 32, + 16, .., + 1 within its 64; the four 64s are
    added in order"""
    t = np.asarray(terms, np.float64)
    lead, n = t.shape[:-1], t.shape[-1]
    groups = max(-(-n // 128), 1)
    v = np.zeros(lead + (groups * 128,), np.float64)
    v[..., :n] = t
    v = v.reshape(lead + (groups, 2, 64))
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    part = v[..., 0, 0] + v[..., 1, 0]                      # (.., groups)
    strands = np.zeros(lead + (256,), np.float64)
    for g0 in range(0, groups, 256):
        blk = part[..., g0:g0 + 256]
        strands[..., :blk.shape[-1]] = strands[..., :blk.shape[-1]] + blk
    s = strands.reshape(lead + (4, 64))
    for off in (32, 16, 8, 4, 2, 1):
        s = s[..., :off] + s[..., off:2 * off]
    s = s[..., 0]
    return ((s[..., 0] + s[..., 1]) + s[..., 2]) + s[..., 3]


def sum_terms(xyz, flags, p0):
    """(10, n) float64: the terms of the ten sums, +0 where the flag is not set"""
    P = np.asarray(xyz, np.float32)
    with np.errstate(all="ignore"):
        e = P.astype(np.float64) - np.asarray(p0, np.float32).astype(np.float64)[None, :]
        t = np.stack([np.ones(len(P)), e[:, 0], e[:, 1], e[:, 2], e[:, 0] * e[:, 0], e[:, 0] * e[:, 1], e[:, 0] * e[:, 2], e[:, 1] * e[:, 1],
                      e[:, 1] * e[:, 2], e[:, 2] * e[:, 2]])
    t[:, ~np.asarray(flags, bool)] = 0.0
    return t


def ten_sums(xyz, flags, p0):
    return tree_sum(sum_terms(xyz, flags, p0))


def plane_from_sums_eigh(sums, p0, prior):
    """rsreg_plane_from_sums with numpy.linalg.eigh for the eigen step, in float64: (normal (3,), d) before any rounding to float, or
    None where the library refuses"""
    s = np.asarray(sums, np.float64)
    m = s[0]
    if not m >= 3.0:
        return None
    mean = s[1:4] / m
    Cm = np.array([[s[4], s[5], s[6]], [s[5], s[7], s[8]], [s[6], s[8], s[9]]]) / m - np.outer(mean, mean)
    if not np.isfinite(Cm).all():
        return None
    w, V = np.linalg.eigh(Cm)
    nrm = V[:, 0] / np.linalg.norm(V[:, 0])
    if nrm @ np.asarray(prior, np.float64)[:3] < 0:
        nrm = -nrm
    return nrm, float(-nrm @ (np.asarray(p0, np.float32).astype(np.float64) + mean))


class Seg:
    """What rsreg_cloud_plane_segment returns, from the reference"""


def segment(api, xyz, distance_threshold=0.0, max_iterations=50, probability=0.99, optimize_coefficients=1, axis=(0.0, 0.0, 0.0), eps_angle=0.0, seed=0,
            batch=256):
    """SACSegmentation::segment.  The eigen step alone goes through api.plane_from_sums (the host solve, held against numpy.linalg.eigh
    in tests/test_plane_seg_cpu.py).  r.min_cs_margin: how near any consumed hypothesis's cs came to cos_eps (inf without an axis)."""
    P = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(P)
    finite = finite_records(P)
    r = Seg()
    on = axis_on(axis, eps_angle)
    r.cos_eps = math.cos(eps_angle) if on else 0.0
    r.found, r.best_hypothesis, r.sample, r.iterations, r.skipped, r.n_inliers, r.refined = False, -1, (-1, -1, -1), 0, 0, 0, False
    r.coeff, r.unrefined, r.sums, r.inliers = np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(NUM_SUMS), np.zeros(0, np.int32)
    r.min_cs_margin, r.counts, r.valid, r.ks = math.inf, [], [], []
    rp = Replay(n, probability, max_iterations)
    model = sample = None
    if n >= 3:
        done = 0
        while rp.wants_more():
            assert done < 11 * max_iterations
            models, samples, valid, cs = hypotheses(P, seed, done, batch, axis, eps_angle)
            counts = count(models, P, distance_threshold)
            for j in range(batch):
                if not rp.wants_more():
                    break
                before = rp.winner
                rp.feed(valid[j], counts[j])
                r.counts.append(int(counts[j]))
                r.valid.append(bool(valid[j]))
                if cs[j] is not None:
                    r.min_cs_margin = min(r.min_cs_margin, abs(cs[j] - r.cos_eps))
                if rp.winner != before:
                    model, sample = models[j].copy(), samples[j].copy()
            done += batch
    r.iterations, r.skipped, r.best, r.ks = rp.it, rp.skipped, rp.best, rp.ks
    if n < 3 or rp.best < 3:
        return r
    r.found, r.best_hypothesis, r.sample, r.unrefined = True, rp.winner, tuple(int(v) for v in sample[:3]), model.copy()
    flags = within(model, P, distance_threshold)[0]
    assert flags.sum() == rp.best
    if optimize_coefficients and flags.sum() >= 3:
        p0 = P[r.sample[0]]
        r.sums = ten_sums(P, flags, p0)
        refined = api.plane_from_sums(r.sums, p0, model)
        if refined is not None:
            model, r.refined = refined, True
            flags = within(model, P, distance_threshold)[0]
    r.coeff, r.flags, r.inliers, r.n_inliers = model, flags, np.flatnonzero(flags).astype(np.int32), int(flags.sum())
    return r
