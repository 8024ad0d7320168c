"""A reference of the radius search of one cloud's records (the queries) in another (the surface) and of what runs on it --
rsreg_cloud_radius_count_surface, rsreg_cloud_normals_radius_surface, rsreg_cloud_fpfh_radius_surface and
rsreg_cloud_spfh_radius_surface as include/rsreg.h defines them -- numpy and scipy only, independent of the engine and built from
the other references by import:

  * search: the finite surface records j with float32 d2(query, j) < float32(float64(radius) * float64(radius)), STRICTLY
    (radius_ref.r2_f32, fitness_ref.d2_f32); candidates from cKDTree.query_ball_point at radius * (1 + 1e-5) in float64, then the
    float32 compare decides.  A query is not a neighbour of anything; a surface record that coincides with it counts; a non-finite
    query has none; m may be 0;
  * normals: radius_ref's covariance with d = neighbour - QUERY in float64 over the m surface neighbours, then eigh, curvature, the
    trace-0 case and the flip towards the viewpoint from the query exactly as radius_ref.normals (normals_ref.cos_view and
    gap_ratio are used); m < 3 and non-finite queries: NaNs;
  * fpfh: the SPFH rows are fpfh_radius_ref.fpfh_radius(surface, surface_normals, radius).spfh -- the surface's own neighbourhoods
    and normals -- kept for the NEEDED surface records (a neighbour of at least one finite query) and zero elsewhere; the weighting
    of fpfh_radius_ref over the surface neighbours with d2 != 0, w = 1.0f / d2 and SPFH[j] * w in float32, added in FLOAT64 one
    after the other in ascending surface record index (order="descending": the other way round); no normal of the query enters;
    NaN rows for a non-finite query and for a query with m = 0, zeros where every neighbour is at distance 0.
fragile_nb: a query with a fragile surface neighbour (fpfh_ref's margin, at the surface's own SPFH rows).
"""
import itertools

import numpy as np
from scipy.spatial import cKDTree

import fpfh_radius_ref as FR
import fpfh_ref as F
import normals_ref as N
import radius_ref as R
from fitness_ref import d2_f32, finite_rows

BINS, ROW = F.BINS, F.ROW


class Neighbours:
    """qfin, sfin: masks of the finite queries / surface records; off (nq + 1), idx: the neighbours of query i are the surface
    records idx[off[i]:off[i + 1]], ascending; I: the query of every pair."""

    def counts(self):
        return np.diff(self.off).astype(np.uint32)


def _xyz(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def search(queries, surface, radius, brute=False):
    """brute: every (finite query, finite surface record) pair goes through the float32 compare, no tree."""
    q, s = _xyz(queries), _xyz(surface)
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError("the radius must be finite and above 0")
    nb = Neighbours()
    nb.qfin, nb.sfin = finite_rows(q), finite_rows(s)
    qi, si = np.flatnonzero(nb.qfin), np.flatnonzero(nb.sfin)
    if len(qi) == 0 or len(si) == 0:
        rows, flat = np.zeros(0, np.int64), np.zeros(0, np.int64)
    elif brute:
        rows, flat = [a.reshape(-1) for a in np.meshgrid(np.arange(len(qi)), np.arange(len(si)), indexing="ij")]
    else:
        with np.errstate(over="ignore"):
            tree = cKDTree(s[si].astype(np.float64))
            cand = tree.query_ball_point(q[qi].astype(np.float64), float(radius) * (1 + 1e-5), return_sorted=True)
        lens = np.fromiter((len(c) for c in cand), np.int64, len(cand))
        flat = np.fromiter(itertools.chain.from_iterable(cand), np.int64, int(lens.sum()))
        rows = np.repeat(np.arange(len(qi)), lens)
    with np.errstate(over="ignore", invalid="ignore"):
        keep = d2_f32(q[qi[rows]], s[si[flat]]) < R.r2_f32(radius)
    nb.I = qi[rows[keep]]
    nb.idx = si[flat[keep]]                      # (ascending inside a query: the tree's order over an ascending `si`)
    nb.off = np.concatenate([[0], np.cumsum(np.bincount(nb.I, minlength=len(q)))]).astype(np.int64)
    return nb


def counts(queries, surface, radius):
    return search(queries, surface, radius).counts()


def normals(queries, surface, radius, viewpoint=(0.0, 0.0, 0.0), nb=None):
    """normals_ref.Normals as radius_ref.normals fills it (m: the surface counts, valid: finite and m >= 3, finite: the finite
    queries), the covariance about the query over its surface neighbours."""
    q, s = _xyz(queries), _xyz(surface)
    nb = nb if nb is not None else search(q, s, radius)
    nq = len(q)
    r = N.Normals()
    r.m = nb.counts()
    d = s.astype(np.float64)[nb.idx] - q.astype(np.float64)[nb.I]
    s1, s2 = np.zeros((nq, 3)), np.zeros((nq, 3, 3))
    np.add.at(s1, nb.I, d)                                  # (unbuffered: one addition after the other, ascending surface index)
    np.add.at(s2, nb.I, d[:, :, None] * d[:, None, :])
    m = np.maximum(r.m, 1).astype(np.float64)
    mean = s1 / m[:, None]
    r.C = s2 / m[:, None, None] - mean[:, :, None] * mean[:, None, :]
    r.finite = nb.qfin
    r.valid = nb.qfin & (r.m >= 3)
    r.trace = np.trace(r.C, axis1=1, axis2=2)
    w, v = np.linalg.eigh(r.C)
    r.evals = w
    n = v[:, :, 0].copy()
    n[r.trace == 0] = (0.0, 0.0, 1.0)
    sm = w.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = np.where((r.trace == 0) | (sm == 0), 0.0, np.abs(w[:, 0] / sm))
    n32 = n.astype(np.float32)
    r.cos = N.cos_view(q, n32, viewpoint)
    with np.errstate(invalid="ignore"):
        n32[r.cos < 0] *= np.float32(-1)
    r.normal = n32
    r.curvature = curv.astype(np.float32)
    r.normal[~r.valid] = np.nan
    r.curvature[~r.valid] = np.nan
    r.gap = N.gap_ratio(w)
    return r


class SurfaceFpfh:
    """m (nq,) uint32; needed (ns,) bool; spfh (ns, 33) float32: the needed rows, zero elsewhere; fragile (ns,) bool: the surface
    records whose SPFH row is fragile; fpfh (nq, 33) float32; H (nq, 33) float64; nan_rows, fragile_nb (nq,) bool."""


def fpfh(queries, surface, surface_normals, radius, order="ascending", nb=None, surface_ref=None):
    """surface_ref: fpfh_radius_ref.fpfh_radius(surface, surface_normals, radius) if the caller holds it already."""
    q, s = _xyz(queries), _xyz(surface)
    nq, ns = len(q), len(s)
    sp = surface_ref if surface_ref is not None else FR.fpfh_radius(s, surface_normals, radius)
    nb = nb if nb is not None else search(q, s, radius)
    r = SurfaceFpfh()
    r.m = nb.counts()
    I, J = nb.I, nb.idx
    r.needed = np.bincount(J, minlength=ns) > 0
    r.spfh = np.where(r.needed[:, None], sp.spfh, np.float32(0)).astype(np.float32)
    r.fragile = sp.fragile
    r.nan_rows = ~nb.qfin | (r.m == 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d2 = d2_f32(q[I], s[J]).astype(np.float32)
        use = np.flatnonzero(d2 != 0)
        if order == "descending":
            use = use[::-1]
        elif order != "ascending":
            raise ValueError(order)
        w = (np.float32(1.0) / d2[use]).astype(np.float32)
        val = (sp.spfh[J[use]] * w[:, None]).astype(np.float32)
        H = np.zeros((nq, ROW), np.float64)
        np.add.at(H, I[use], val.astype(np.float64))          # (unbuffered: one addition after the other, in the order of `use`)
        H3 = H.reshape(nq, 3, BINS)
        S = H3[:, :, 0].copy()
        for bb in range(1, BINS):
            S = S + H3[:, :, bb]
        scale = np.where(S != 0, 100.0 / S, 0.0)
        out = (H3 * scale[:, :, None]).astype(np.float32).reshape(nq, ROW)
    out[r.nan_rows] = np.nan
    r.H, r.fpfh = H, out
    r.fragile_nb = np.bincount(I, weights=sp.fragile[J], minlength=nq) > 0
    return r
