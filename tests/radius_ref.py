"""A reference of the exact radius search (rsreg_cloud_radius_count), of pcl::RadiusOutlierRemoval
(rsreg_cloud_radius_outlier_removal) and of pcl::NormalEstimation with setRadiusSearch (rsreg_cloud_normals_radius) as
include/rsreg.h defines them, numpy and scipy's cKDTree only, independent of the engine:

  * the search runs over the finite records only; record j is a neighbour of record i when d2(i, j) < r2, STRICTLY, with d2 the
    float32 squared distance ((dx*dx + dy*dy) + dz*dz, fitness_ref.d2_f32) and r2 = float32(float64(radius) * float64(radius));
    the record itself and exact copies are neighbours like any other; a non-finite record has none;
  * candidates come from cKDTree.query_ball_point in float64 with a generous margin (radius * (1 + 1e-5): float32 rescoring moves a
    squared distance by a few ulp, 1e-7 relative), then the exact float32 compare decides -- never an n x n table;
  * exact copies ask the same question and get the same answer: it is answered once per distinct point (a raw frame's thousands
    of missing-depth records at the origin are one query), and the answers are expanded to the records where a caller needs them;
  * RadiusOutlierRemoval: removed when count <= min_neighbors (negative: when count > min_neighbors), non-finite records by the
    same rule with their count of 0; kept records keep their order;
  * the normal of a record with m >= 3 neighbours: d = neighbour - record in float64, C = (sum d d^T) / m - (sum d / m)(sum d / m)^T,
    then np.linalg.eigh, curvature, the trace-0 case and the flip exactly as normals_ref.normals (its cos_view and gap_ratio are
    used); m < 3 and non-finite records: NaNs.
"""
import itertools

import numpy as np
from scipy.spatial import cKDTree

import normals_ref as N
from fitness_ref import d2_f32, finite_rows


def r2_f32(radius):
    """KdTreeFLANN::radiusSearch's cast: the float of the double product."""
    with np.errstate(over="ignore"):
        return np.float32(np.float64(radius) * np.float64(radius))


class Neighbours:
    """fin: mask of the finite records; orig: their original indices; inv: finite record -> its distinct point; off (q + 1), idx:
    the neighbours of distinct point u are the ORIGINAL record indices idx[off[u]:off[u + 1]], ascending."""

    def counts(self):
        """uint32 per record: its neighbours, itself among them; 0 for a non-finite record."""
        c = np.zeros(len(self.fin), np.uint32)
        c[self.fin] = np.diff(self.off)[self.inv].astype(np.uint32)
        return c


def search(xyz, radius, workers=-1):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError("the radius must be finite and above 0")
    nb = Neighbours()
    nb.fin = finite_rows(xyz)
    nb.orig = np.flatnonzero(nb.fin)
    t = xyz[nb.fin]
    nb.q, inv = np.unique(t, axis=0, return_inverse=True) if len(t) else (t, np.zeros(0, np.int64))
    nb.inv = inv.reshape(-1)
    if len(t) == 0:
        nb.off, nb.idx = np.zeros(1, np.int64), np.zeros(0, np.int64)
        return nb
    tree = cKDTree(t.astype(np.float64))
    cand = tree.query_ball_point(nb.q.astype(np.float64), float(radius) * (1 + 1e-5), return_sorted=True, workers=workers)
    lens = np.fromiter((len(c) for c in cand), np.int64, len(cand))
    flat = np.fromiter(itertools.chain.from_iterable(cand), np.int64, int(lens.sum()))
    rows = np.repeat(np.arange(len(nb.q)), lens)
    r2 = r2_f32(radius)
    keep = np.zeros(len(flat), bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, len(flat), 1 << 22):
            e = s + (1 << 22)
            keep[s:e] = d2_f32(nb.q[rows[s:e]], t[flat[s:e]]) < r2
    nb.off = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=len(nb.q)))]).astype(np.int64)
    nb.idx = nb.orig[flat[keep]]            # (sorted by the tree's index inside a row, and orig is ascending)
    return nb


def counts(xyz, radius):
    return search(xyz, radius).counts()


def ror_keep(count, min_neighbors, negative=False):
    """The records pcl::RadiusOutlierRemoval keeps, from their counts."""
    if min_neighbors < 0:
        raise ValueError("min_neighbors must not be negative")
    above = np.asarray(count).astype(np.int64) > int(min_neighbors)
    return ~above if negative else above


def covariances(xyz, nb):
    """(C (n, 3, 3) float64, m (n,) counts): the covariance of every finite record's neighbours about the record itself (zeros where
    m is 0: nothing to sum)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    p = xyz.astype(np.float64)
    nq = len(nb.q)
    lens = np.diff(nb.off)
    Cq = np.zeros((nq, 3, 3))
    if nq:
        rows = np.repeat(np.arange(nq), lens)
        d = p[nb.idx] - nb.q.astype(np.float64)[rows]
        first = nb.off[:-1]                                   # (every distinct point has itself: no empty row)
        s1 = np.add.reduceat(d, first, axis=0)
        s2 = np.add.reduceat(d[:, :, None] * d[:, None, :], first, axis=0)
        m = lens.astype(np.float64)
        mean = s1 / m[:, None]
        Cq = s2 / m[:, None, None] - mean[:, :, None] * mean[:, None, :]
    C = np.zeros((len(xyz), 3, 3))
    C[nb.fin] = Cq[nb.inv]
    return C, nb.counts()


def normals(xyz, radius, viewpoint=(0.0, 0.0, 0.0), nb=None):
    """normals_ref.Normals with m (the counts) and valid (finite and m >= 3) beside its fields; `finite` is the finite mask."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    nb = nb if nb is not None else search(xyz, radius)
    r = N.Normals()
    r.C, r.m = covariances(xyz, nb)
    r.finite = nb.fin
    r.valid = nb.fin & (r.m >= 3)
    r.trace = np.trace(r.C, axis1=1, axis2=2)
    w, v = np.linalg.eigh(r.C)
    r.evals = w
    n = v[:, :, 0].copy()
    n[r.trace == 0] = (0.0, 0.0, 1.0)
    s = w.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = np.where((r.trace == 0) | (s == 0), 0.0, np.abs(w[:, 0] / s))
    n32 = n.astype(np.float32)
    r.cos = N.cos_view(xyz, n32, viewpoint)
    with np.errstate(invalid="ignore"):
        n32[r.cos < 0] *= np.float32(-1)
    r.normal = n32
    r.curvature = curv.astype(np.float32)
    r.normal[~r.valid] = np.nan
    r.curvature[~r.valid] = np.nan
    r.gap = N.gap_ratio(w)
    return r
