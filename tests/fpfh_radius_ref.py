"""A reference of pcl::FPFHEstimationOMP with setRadiusSearch as include/rsreg.h defines it (rsreg_cloud_spfh_radius,
rsreg_cloud_fpfh_radius), numpy and scipy only, independent of the engine and built from pieces the other references hold:

  * the neighbourhoods are radius_ref.search's: float32 d2 < float32(radius * radius), strictly, the record itself and exact copies
    among them, no cap; m is their number;
  * the pair features, the bins and the margins are fpfh_ref's (float64, nothing contracted); a pair is not counted when j == i,
    when the points coincide, when dp is parallel to the source normal or when a normal is not finite;
  * a bin hit by c pairs holds 0.0f + hist_incr, c times, in float32, hist_incr = 100.0f / float32(m - 1): per distinct m the table
    np.cumsum(np.full(m - 1, incr, float32), dtype=float32), which adds one after the other;
  * the weighting: w = 1.0f / d2 and val = SPFH[j] * w in float32 for every neighbour with d2 != 0, added in FLOAT64 one after the
    other in ascending record index (order="descending": the other way round, for the test that counts what the order can move);
    S_t = the eleven sums of block t added in ascending bin order; out = float32(H * (100 / S_t)), 0 where S_t is 0.

FRAGILE and fragile_nb are fpfh_ref's, at the same margin of 1e-9 bins, which is derived there and not measured.
"""
import numpy as np

import fpfh_ref as F
import radius_ref as R
from fitness_ref import d2_f32

BINS, ROW = F.BINS, F.ROW


class FpfhRadius:
    """m (n,) uint32; I, J: the pairs (record, neighbour), J ascending inside a record, the record itself among them; d2 per pair;
    valid per pair: counted; scaled per pair (., 3); counts (n, 33) int; spfh, fpfh (n, 33) float32; H (n, 33) float64: the sums
    before they are normalised; fragile, fragile_nb, nan_rows (n,) bool."""


def spfh_rows(counts, m):
    """(n, 33) float32 from the integer counts and the neighbour counts: the sequential float32 sum, a table per distinct m."""
    out = np.zeros(counts.shape, np.float32)
    for mv in np.unique(m):
        if mv < 2:
            continue                                   # m == 1: no pair, no addition; m == 0: not a finite record
        incr = np.float32(100.0) / np.float32(mv - 1)
        tab = np.concatenate([np.zeros(1, np.float32), np.cumsum(np.full(int(mv) - 1, incr, np.float32), dtype=np.float32)])
        rows = m == mv
        out[rows] = tab[counts[rows]]
    return out


def fpfh_radius(xyz, normals, radius, order="ascending", nb=None):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(np.asarray(normals, np.float32)[:, :3])
    n = len(xyz)
    if len(nrm) != n:
        raise ValueError("one normal per record")
    nb = nb if nb is not None else R.search(xyz, radius)
    r = FpfhRadius()
    r.m = nb.counts()
    lens = np.diff(nb.off)[nb.inv] if len(nb.inv) else np.zeros(0, np.int64)
    r.I = np.repeat(nb.orig, lens)
    first = np.repeat(nb.off[:-1][nb.inv] if len(nb.inv) else np.zeros(0, np.int64), lens)
    within = np.arange(len(r.I)) - np.repeat(np.cumsum(lens) - lens, lens)
    r.J = nb.idx[first + within]
    I, J = r.I, r.J
    scaled, valid = F.pair_features(xyz[I], nrm[I], xyz[J], nrm[J])
    valid = valid & (I != J)
    r.valid, r.scaled = valid, scaled
    margin = np.where(valid, F.margins_of(scaled), np.inf)
    b = F.bins_of(scaled) + np.arange(3) * BINS
    flat = (I[:, None] * ROW + b)[valid]
    r.counts = np.bincount(flat.reshape(-1), minlength=n * ROW).reshape(n, ROW)
    r.spfh = spfh_rows(r.counts, r.m)
    fin = r.m > 0
    r.nan_rows = ~fin | ~np.isfinite(nrm).all(axis=1)

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r.d2 = d2_f32(xyz[I], xyz[J]).astype(np.float32)
        use = np.flatnonzero(r.d2 != 0)
        if order == "descending":
            use = use[::-1]
        elif order != "ascending":
            raise ValueError(order)
        w = (np.float32(1.0) / r.d2[use]).astype(np.float32)
        val = (r.spfh[J[use]] * w[:, None]).astype(np.float32)
        H = np.zeros((n, ROW), np.float64)
        np.add.at(H, I[use], val.astype(np.float64))          # (unbuffered: one addition after the other, in the order of `use`)
        H3 = H.reshape(n, 3, BINS)
        S = H3[:, :, 0].copy()
        for bb in range(1, BINS):
            S = S + H3[:, :, bb]
        scale = np.where(S != 0, 100.0 / S, 0.0)
        out = (H3 * scale[:, :, None]).astype(np.float32).reshape(n, ROW)
    out[r.nan_rows] = np.nan
    r.H, r.fpfh = H, out
    r.fragile = np.bincount(I, weights=margin < F.FRAGILE_BELOW, minlength=n) > 0
    r.fragile_nb = r.fragile | (np.bincount(I, weights=r.fragile[J], minlength=n) > 0)
    return r


def ulp_apart(a, b):
    """The distance in float32 steps between two arrays of finite floats of one sign."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
