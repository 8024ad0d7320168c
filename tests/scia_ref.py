"""The numpy reference of the SampleConsensusInitialAlignment contract (include/rsreg.h: rsreg_cloud_error_transforms,
rsreg_cloud_initial_alignment_hypotheses, rsreg_cloud_initial_alignment).  The float32 transform, the brute-force nearest distance and
the sum tree are tests/prerej_ref.py's, the generator and the float32 distance tests/sac_ref.py's, the solve api.umeyama_from_sums
(the host solve, which is not code under test); new here are the two error functors, the sequential sampler and the selection replay.

Nothing here knows about batches, tiles, slices or a grid: a hypothesis is a function of (seed, h), an error a function of
(T, source, target, functor, thr).
"""
import numpy as np

import sac_ref as S
from prerej_ref import nearest_d2, sum_tree, xform, xyz_of

TRUNCATED, HUBER = 0, 1
DRAWS, MAX_SAMPLES = 56, 8
DEFAULT_DISTANCE = float(np.sqrt(np.finfo(np.float64).max))


def draw_index(seed, h, draw, n):
    return S.draw_index(seed, h, draw, n)


def threshold(max_correspondence_distance):
    """thr: the float the SQUARED distances are compared with"""
    with np.errstate(over="ignore"):
        return np.float32(max_correspondence_distance)


def truncated_terms(e, thr):
    """float64 per e (float32): (e < +inf and e <= thr) ? (double)(e / thr) : 1.0, the division in float32"""
    e, thr = np.asarray(e, np.float32), np.float32(thr)
    with np.errstate(all="ignore"):
        q = (e / thr).astype(np.float32)
        assert q.dtype == np.float32
        return np.where(np.isfinite(e) & (e <= thr), q.astype(np.float64), 1.0)


def huber_terms(e, thr):
    """float64 per e (float32): e <= thr ? (0.5 * e) * e : (0.5 * thr) * (2.0 * e - thr) in double"""
    e, t = np.asarray(e, np.float32).astype(np.float64), np.float64(np.float32(thr))
    with np.errstate(all="ignore"):
        return np.where(e <= t, (0.5 * e) * e, (0.5 * t) * (2.0 * e - t))


def terms(e, fn, thr):
    return truncated_terms(e, thr) if fn == TRUNCATED else huber_terms(e, thr)


def nearest(T, src, tgt):
    """(e float32 per source record, which records are finite): e = +inf where p' is not finite or the target has no finite record"""
    src, tgt = xyz_of(src), xyz_of(tgt)
    e = np.full(len(src), np.inf, np.float32)
    fin = np.isfinite(src).all(axis=1)
    if fin.any():
        e[fin] = nearest_d2(xform(T, src[fin]), tgt)
    return e, fin


def error(T, src, tgt, fn, max_correspondence_distance):
    """the contract's error of one transform"""
    e, fin = nearest(T, src, tgt)
    return sum_tree(np.where(fin, terms(e, fn, threshold(max_correspondence_distance)), 0.0))


def error_transforms(Ts, src, tgt, fn, max_correspondence_distance):
    Ts = np.asarray(Ts, np.float32).reshape(-1, 4, 4)
    if len(xyz_of(src)) == 0:
        return np.zeros(len(Ts), np.float64)
    return np.array([error(T, src, tgt, fn, max_correspondence_distance) for T in Ts], np.float64)


def sampler(src, nbr, seed, h, nr_samples, min_sample_distance):
    """(the accepted records in order, at most nr_samples of them; the draw at which each was accepted)"""
    ns = len(src)
    msd2 = float(min_sample_distance) * float(min_sample_distance)
    ids, draws = [], []
    for d in range(DRAWS):
        if len(ids) == nr_samples:
            break
        c = int(draw_index(seed, h, d, ns))
        if nbr[c, 0] < 0 or not np.isfinite(src[c]).all() or c in ids:
            continue
        if not all(float(S.l2_simple(src[c], src[s])) >= msd2 for s in ids):
            continue
        ids.append(c)
        draws.append(d)
    return ids, draws


def pair_sums(P, Q):
    """the 17 sums of the pairs in float64, each 0.0 + the terms in pair order"""
    s = np.zeros(S.NUM_SUMS, np.float64)
    for p32, q32 in zip(P, Q):
        p, q = p32.astype(np.float64), q32.astype(np.float64)
        s[0] += 1.0
        s[1:4] += p
        s[4:7] += q
        s[7:16] += np.outer(q, p).ravel()
        s[16] += np.float64(S.l2_simple(p32, q32))
    return s


def hypothesis(api, src, tgt, nbr, seed, h, nr_samples=3, min_sample_distance=0.0):
    """(T 4 x 4 float32 or None, the 16 sample words): hypothesis h of the contract"""
    words = np.full(16, -1, np.int32)
    ns, k = nbr.shape
    if ns == 0:
        return None, words
    ids, _ = sampler(src, nbr, seed, h, nr_samples, min_sample_distance)
    if len(ids) < nr_samples:
        return None, words
    match = [int(nbr[ids[j], int(draw_index(seed, h, DRAWS + j, k))]) for j in range(nr_samples)]
    words[:nr_samples], words[8:8 + nr_samples] = ids, match
    P, Q = src[ids], tgt[match]
    if not np.isfinite(Q).all():
        return None, words
    try:
        with np.errstate(all="ignore"):
            T = api.umeyama_from_sums(pair_sums(P, Q))
    except Exception:
        T = None
    return T, words


def hypotheses(api, src, tgt, nbr, seed, first, count, nr_samples=3, min_sample_distance=0.0):
    """(transforms (count, 4, 4) NaN where invalid, valid, samples (count, 16)) of rsreg_cloud_initial_alignment_hypotheses"""
    src, tgt, nbr = xyz_of(src), xyz_of(tgt), np.asarray(nbr, np.int32)
    Ts, valid, words = np.full((count, 4, 4), np.nan, np.float32), np.zeros(count, bool), np.full((count, 16), -1, np.int32)
    for j in range(count):
        T, words[j] = hypothesis(api, src, tgt, nbr, seed, first + j, nr_samples, min_sample_distance)
        if T is not None:
            Ts[j], valid[j] = T, True
    return Ts, valid, words


class Scia:
    """What rsreg_cloud_initial_alignment returns, from the reference"""


def initial_alignment(api, src, tgt, nbr, guess=None, max_correspondence_distance=DEFAULT_DISTANCE, min_sample_distance=0.0, nr_samples=3,
                      error_function=TRUNCATED, max_iterations=10, seed=0, scores=None):
    """scores (optional): a function (Ts) -> errors in place of the brute-force error of each valid hypothesis (for the cases whose
    many hypotheses are few DISTINCT transforms)"""
    src, tgt, nbr = xyz_of(src), xyz_of(tgt), np.asarray(nbr, np.int32)
    r = Scia()
    r.transform, r.found, r.best_hypothesis, r.sample, r.match = np.eye(4, dtype=np.float32), False, -1, (-1,) * 8, (-1,) * 8
    r.n_valid, r.error, r.errors = 0, np.inf, np.full(max_iterations, np.nan)
    H = max(max_iterations - 1, 0) if guess is not None else max_iterations
    r.valid = np.zeros(H, bool)
    if len(src) == 0:
        return r
    held, lowest = False, np.inf
    if guess is not None:
        g = np.asarray(guess, np.float32).reshape(4, 4)
        e = error(g, src, tgt, error_function, max_correspondence_distance)
        r.error = e
        if not np.isnan(e):
            held, lowest = True, e
        if np.isfinite(e):
            r.transform = g.copy()
    Ts, valid, words = hypotheses(api, src, tgt, nbr, seed, 0, H, nr_samples, min_sample_distance)
    r.valid, r.n_valid = valid, int(valid.sum())
    idx = np.flatnonzero(valid)
    if len(idx):
        errs = scores(Ts[idx]) if scores else error_transforms(Ts[idx], src, tgt, error_function, max_correspondence_distance)
        r.errors[idx] = errs
    for h in idx:
        e = r.errors[h]
        if (not e < lowest) if held else np.isnan(e):
            continue
        held, lowest = True, e
        r.found, r.best_hypothesis, r.transform, r.error = True, int(h), Ts[h], float(e)
        r.sample, r.match = tuple(int(v) for v in words[h, :8]), tuple(int(v) for v in words[h, 8:])
    return r
