"""The numpy reference of the pose-from-descriptor-neighbours contract (include/rsreg.h: rsreg_cloud_score_transforms,
rsreg_cloud_prerejective, pcl::SampleConsensusPrerejective).  The generator, the float32 distance and the three-pair sums are
tests/sac_ref.py's (draw_index, l2_simple, three_pair_sums, and the host solve api.umeyama_from_sums, which is not code under test);
new here are a float32 brute-force nearest distance, the sum tree written out step by step, the polygon test and the selection replay.

Nothing here knows about batches, tiles, slices or a grid: a hypothesis is a function of (seed, h), a score a function of
(T, source, target, range).
"""
import numpy as np

import sac_ref as S

WAVE, GROUP = 64, 128


def xyz_of(points):
    return np.ascontiguousarray(points, np.float32).reshape(-1, 3)


def xform(T, P):
    """(n, 3) float32: P moved by the 4 x 4 T in transformPointCloud's order, every operation rounded once"""
    m = np.asarray(T, np.float32).reshape(4, 4)
    with np.errstate(all="ignore"):
        out = []
        for r in range(3):
            a = (m[r, 0] * P[:, 0]).astype(np.float32) + (m[r, 1] * P[:, 1]).astype(np.float32)
            a = a.astype(np.float32) + (m[r, 2] * P[:, 2]).astype(np.float32)
            out.append((a.astype(np.float32) + m[r, 3]).astype(np.float32))
    return np.stack(out, axis=1)


def nearest_d2(Q, tgt, chunk=256):
    """float32 per query: the smallest L2_Simple squared distance to the finite records of tgt by brute force (+inf: there is none, or
    the query is not finite)"""
    tgt = tgt[np.isfinite(tgt).all(axis=1)]
    out = np.full(len(Q), np.inf, np.float32)
    ok = np.isfinite(Q).all(axis=1)
    if len(tgt) == 0:
        return out
    idx = np.flatnonzero(ok)
    for a in range(0, len(idx), chunk):
        q = Q[idx[a:a + chunk]]
        d2 = S.l2_simple(q[:, None, :], tgt[None, :, :])
        assert d2.dtype == np.float32
        with np.errstate(all="ignore"):
            out[idx[a:a + chunk]] = np.fmin.reduce(d2, axis=1)   # (fmin: a NaN never wins)
    return out


def sum_tree(terms):
    """the contract's sum of ns float64 terms: term i is lane i % 64 of wave (i / 64) % 2 of group i / 128, zeros behind the last;
    six pairwise halvings across lane bit 5 .. 0, wave 0 + wave 1, the groups accumulated in ascending order"""
    terms = np.asarray(terms, np.float64)
    groups = max(1, -(-len(terms) // GROUP))
    v = np.zeros(groups * GROUP, np.float64)
    v[:len(terms)] = terms
    v = v.reshape(groups, 2, WAVE)
    for half in (32, 16, 8, 4, 2, 1):
        v = v[..., :half] + v[..., half:2 * half]
    g = v[:, 0, 0] + v[:, 1, 0]
    return float(np.add.accumulate(g)[-1])


def sum_tree_depth(ns):
    """the most additions one term passes through: 6 in its wave, 1 for the group, one per group behind the first"""
    return 6 + 1 + max(0, -(-ns // GROUP) - 1)


def score(T, src, tgt, max_range):
    """(count, sum, flags, d2) of one transform: the contract's score of every source record"""
    src, tgt = xyz_of(src), xyz_of(tgt)
    d2 = np.full(len(src), np.inf, np.float32)
    fin = np.isfinite(src).all(axis=1)
    if fin.any():
        d2[fin] = nearest_d2(xform(T, src[fin]), tgt)
    with np.errstate(all="ignore"):
        flags = d2.astype(np.float64) < float(max_range) * float(max_range)
    return int(flags.sum()), sum_tree(np.where(flags, d2.astype(np.float64), 0.0)), flags, d2


def score_transforms(Ts, src, tgt, max_range):
    """(counts uint32, sums float64) of rsreg_cloud_score_transforms"""
    Ts = np.asarray(Ts, np.float32).reshape(-1, 4, 4)
    rows = [score(T, src, tgt, max_range)[:2] for T in Ts]
    return np.array([c for c, _ in rows], np.uint32), np.array([s for _, s in rows], np.float64)


def polygon_ok(P, Q, similarity_threshold):
    """the polygon test over three pairs (P source points, Q target points), float32"""
    sim2 = np.float32(similarity_threshold) * np.float32(similarity_threshold)
    assert sim2.dtype == np.float32
    with np.errstate(all="ignore"):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            ds, dt = S.l2_simple(P[a], P[b]), S.l2_simple(Q[a], Q[b])
            sim = ds / dt if ds < dt else dt / ds
            assert np.asarray(sim).dtype == np.float32
            if not sim >= sim2:
                return False
    return True


def polygon_edges(P, Q):
    """(3, 3) float32, a row (ds, dt, sim) per edge as polygon_ok forms them -- all three edges, whether or not an earlier one fails;
    for tests/test_prerej_edges_cpu.py, which classifies them (a denormal, 0, +inf, a NaN sim)"""
    out = np.zeros((3, 3), np.float32)
    with np.errstate(all="ignore"):
        for e, (a, b) in enumerate(((0, 1), (1, 2), (2, 0))):
            ds, dt = S.l2_simple(P[a], P[b]), S.l2_simple(Q[a], Q[b])
            sim = ds / dt if ds < dt else dt / ds
            assert np.asarray(sim).dtype == np.float32
            out[e] = ds, dt, sim
    return out


def sample_edges(src, tgt, nbr, seed, h):
    """polygon_edges of hypothesis h's sample, or None when its draws do not give three distinct eligible records that are finite on
    both sides (hypothesis() ends before the polygon test there)"""
    ns, k = nbr.shape
    ids = [int(S.draw_index(seed, h, d, ns)) for d in range(3)]
    if any(nbr[i, 0] < 0 for i in ids) or len(set(ids)) < 3:
        return None
    match = [int(nbr[ids[d], int(S.draw_index(seed, h, 3 + d, k))]) for d in range(3)]
    P, Q = src[ids], tgt[match]
    if not (np.isfinite(P).all() and np.isfinite(Q).all()):
        return None
    return polygon_edges(P, Q)


def hypothesis(api, src, tgt, nbr, seed, h, similarity_threshold):
    """(T 4 x 4 float32 or None, the three source records, the three target records or None): hypothesis h of the contract"""
    ns, k = nbr.shape
    ids = [int(S.draw_index(seed, h, d, ns)) for d in range(3)]
    cols = [int(S.draw_index(seed, h, 3 + d, k)) for d in range(3)]
    if any(nbr[i, 0] < 0 for i in ids):
        return None, tuple(ids), None
    match = [int(nbr[ids[d], cols[d]]) for d in range(3)]
    if len(set(ids)) < 3:
        return None, tuple(ids), tuple(match)
    P, Q = src[ids], tgt[match]
    if not (np.isfinite(P).all() and np.isfinite(Q).all()) or not polygon_ok(P, Q, similarity_threshold):
        return None, tuple(ids), tuple(match)
    try:
        T = api.umeyama_from_sums(S.three_pair_sums(P, Q, range(3)))
    except Exception:
        T = None
    return T, tuple(ids), tuple(match)


def select(counts, sums, valid, ns, inlier_fraction=0.0, select_by_inliers=0):
    """(winner or -1, its error): the selection replayed in hypothesis order"""
    best, best_c, best_e = -1, 0, 0.0
    for h in range(len(counts)):
        c = int(counts[h])
        if not valid[h] or c < 1 or not (float(c) / float(ns) >= inlier_fraction):
            continue
        e = float(sums[h]) / float(c)
        if best < 0:
            better = True
        elif select_by_inliers:
            better = c > best_c or (c == best_c and e < best_e)
        else:
            better = e < best_e
        if better:
            best, best_c, best_e = h, c, e
    return best, best_e


class Prerej:
    """What rsreg_cloud_prerejective returns, from the reference"""


def prerejective(api, src, tgt, nbr, max_iterations=10, similarity_threshold=0.9, max_correspondence_distance=None, inlier_fraction=0.0,
                 select_by_inliers=0, seed=0):
    src, tgt = xyz_of(src), xyz_of(tgt)
    nbr = np.asarray(nbr, np.int32)
    ns = len(src)
    rng = np.sqrt(np.finfo(np.float64).max) if max_correspondence_distance is None else max_correspondence_distance
    r = Prerej()
    r.transform, r.found, r.best_hypothesis, r.sample, r.match = np.eye(4, dtype=np.float32), False, -1, (-1, -1, -1), (-1, -1, -1)
    r.n_valid, r.n_inliers, r.fitness, r.inliers = 0, 0, 0.0, np.zeros(0, np.int32)
    r.counts, r.sums, r.valid = np.zeros(max_iterations, np.uint32), np.zeros(max_iterations), np.zeros(max_iterations, bool)
    if ns == 0 or len(tgt) == 0:
        return r
    hyps, flags = [], {}
    for h in range(max_iterations):
        T, ids, match = hypothesis(api, src, tgt, nbr, seed, h, similarity_threshold)
        hyps.append((T, ids, match))
        if T is not None:
            r.valid[h] = True
            r.counts[h], r.sums[h], flags[h], _ = score(T, src, tgt, rng)
    r.n_valid = int(r.valid.sum())
    w, err = select(r.counts, r.sums, r.valid, ns, inlier_fraction, select_by_inliers)
    if w < 0:
        return r
    r.found, r.best_hypothesis, r.transform, r.sample, r.match = True, w, hyps[w][0], hyps[w][1], hyps[w][2]
    r.n_inliers, r.fitness, r.inliers = int(r.counts[w]), err, np.flatnonzero(flags[w]).astype(np.int32)
    return r
