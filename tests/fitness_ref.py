"""A reference of Registration::getFitnessScore(max_range) (PCL 1.9 registration.hpp), independent of the engine:

  * positions: the source records moved by the final transform (the caller hands them in, from rsreg_transform_cloud or
    filters_ref.transform: x' = ((m00*x + m01*y) + m02*z) + m03 in float32);
  * for each finite position the float32 squared distance ((dx*dx + dy*dy) + dz*dz) to its nearest finite target point --
    chunked brute force up to 2^24 pairs, beyond that cKDTree candidates rescored in float32 until every row is closed;
  * a record counts if double(d2) <= max_range (PCL's quirk: the range is compared with the SQUARED distance);
  * the counted d2 summed in float64 one after the other, in record order; DBL_MAX when none counts.
"""
import sys

import numpy as np
from scipy.spatial import cKDTree

DBL_MAX = sys.float_info.max
_BRUTE = 1 << 24   # query x target pairs the chunked brute force takes; beyond: the tree


def d2_f32(q, t):
    """FLANN L2_Simple<float> between rows of q and rows of t (broadcast), every step rounded to float32."""
    d = (q - t).astype(np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def finite_rows(a):
    return np.isfinite(a).all(axis=1)


def nearest_d2_brute(q, tgt, chunk=256):
    """float32 nearest squared distance of every row of q (inf: non-finite row or no finite target)."""
    q = np.ascontiguousarray(q, np.float32)
    t = np.ascontiguousarray(tgt, np.float32)
    t = t[finite_rows(t)]
    out = np.full(len(q), np.inf, np.float32)
    ok = np.flatnonzero(finite_rows(q))
    if len(t) == 0:
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, len(ok), chunk):
            rows = ok[s:s + chunk]
            out[rows] = d2_f32(q[rows, None, :], t[None, :, :]).min(axis=1)
    return out


def nearest_d2_tree(q, tgt, k0=8):
    """The same as nearest_d2_brute through cKDTree candidates: a row is closed once the float64 distance of its last candidate
    lies clearly beyond the best float32 d2 (float32 rescoring moves a distance by a few ulp at most)."""
    q = np.ascontiguousarray(q, np.float32)
    t = np.ascontiguousarray(tgt, np.float32)
    t = np.unique(t[finite_rows(t)], axis=0)   # (copies of a target point would tie every candidate list they fill)
    out = np.full(len(q), np.inf, np.float32)
    fin = np.flatnonzero(finite_rows(q))
    if len(t) == 0 or len(fin) == 0:
        return out
    uq, inv = np.unique(q[fin], axis=0, return_inverse=True)   # (copies of a query are searched once)
    out[fin] = _tree_rows(uq, t, k0)[inv.reshape(-1)]
    return out


def _tree_rows(q, t, k0):
    out = np.full(len(q), np.inf, np.float32)
    todo = np.arange(len(q))
    tree = cKDTree(t.astype(np.float64))
    k = min(k0, len(t))
    while len(todo):
        dist, idx = tree.query(q[todo].astype(np.float64), k)
        dist, idx = dist.reshape(len(todo), -1), idx.reshape(len(todo), -1)
        with np.errstate(over="ignore", invalid="ignore"):
            best = d2_f32(q[todo][:, None, :], t[idx]).min(axis=1)
        closed = (k >= len(t)) | (dist[:, -1] ** 2 > best.astype(np.float64) * (1 + 1e-5) + 1e-30)
        out[todo[closed]] = best[closed]
        todo = todo[~closed]
        k = min(4 * k, len(t))
    return out


def nearest_d2(q, tgt):
    if len(q) * len(tgt) <= _BRUTE:
        return nearest_d2_brute(q, tgt)
    return nearest_d2_tree(q, tgt)


def fitness(pos, tgt, max_range=DBL_MAX, valid=None):
    """(score, records in range).  pos: (n, 3) float32 source positions at the final pose; valid (optional): which records were
    finite before the transform (a non-finite record is never counted)."""
    d = nearest_d2(pos, tgt)
    keep = np.isfinite(d) & (d.astype(np.float64) <= max_range)
    if valid is not None:
        keep &= valid
    vals = d[keep].astype(np.float64)
    if len(vals) == 0:
        return DBL_MAX, 0
    return float(np.cumsum(vals)[-1]) / len(vals), int(len(vals))


def fitness_sums(pos, tgt, max_range=DBL_MAX, valid=None):
    """(count, sum of d2) as rsreg_icp_fitness_sums reports them."""
    d = nearest_d2(pos, tgt)
    keep = np.isfinite(d) & (d.astype(np.float64) <= max_range)
    if valid is not None:
        keep &= valid
    vals = d[keep].astype(np.float64)
    return float(len(vals)), float(np.cumsum(vals)[-1]) if len(vals) else 0.0
