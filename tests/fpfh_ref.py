"""A reference of pcl::FPFHEstimation with setKSearch as include/rsreg.h defines it (rsreg_cloud_spfh, rsreg_cloud_fpfh), numpy
only, independent of the engine:

  * the neighbourhoods are normals_ref.knn's: float32 squared distances, the first k by (d2, original index), the record itself
    among them;
  * the pair features in float64 from the float32 inputs, every product and sum an operation of its own (numpy contracts
    nothing), the dot products as (x + y) + z, the cross products component by component;
  * the bins: floor of the scaled features, clamped to [0, 10]; the counts are integers;
  * a bin hit by c pairs holds 0.0f + hist_incr, c times, in float32 (a table);
  * the FPFH sums in float32 in PCL's order: neighbour by neighbour, feature by feature, bin by bin.

For every pair the reference also returns a MARGIN: the distance, in bins, of each scaled feature to the nearest interior edge
1 .. 10, for f1 to 0 and 11 as well (theta = +-pi wraps from bin 10 to bin 0 on the sign of a zero).  A record is FRAGILE when one
of its pairs has a margin below 1e-9 bins: two correctly working atan2's differ by about 1e-15 rad, the other operations are
correctly rounded in both implementations, so the margin is generous by six orders.  It is derived, not measured.
"""
import numpy as np

import normals_ref as N

BINS = 11
ROW = 3 * BINS
FRAGILE_BELOW = 1e-9
PI = np.pi
INV_TWO_PI = 1.0 / (2.0 * np.pi)


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _cross(ax, ay, az, bx, by, bz):
    return ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx


def pair_features(pi, ni, pj, nj):
    """pi, ni, pj, nj: (..., 3) float32 -> (scaled (..., 3) float64: the three features in bins, valid (...) bool).  A pair is
    not valid when the points coincide, when dp is parallel to the source normal, or when a normal is not finite."""
    pi, ni, pj, nj = (np.asarray(a, np.float32).astype(np.float64) for a in (pi, ni, pj, nj))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dx, dy, dz = pj[..., 0] - pi[..., 0], pj[..., 1] - pi[..., 1], pj[..., 2] - pi[..., 2]
        f4 = np.sqrt((dx * dx + dy * dy) + dz * dz)
        n1x, n1y, n1z = ni[..., 0], ni[..., 1], ni[..., 2]
        n2x, n2y, n2z = nj[..., 0], nj[..., 1], nj[..., 2]
        a1 = _dot(n1x, n1y, n1z, dx, dy, dz) / f4
        a2 = _dot(n2x, n2y, n2z, dx, dy, dz) / f4
        swap = np.abs(a1) < np.abs(a2)
        f3 = np.where(swap, -a2, a1)
        n1x, n2x = np.where(swap, n2x, n1x), np.where(swap, n1x, n2x)
        n1y, n2y = np.where(swap, n2y, n1y), np.where(swap, n1y, n2y)
        n1z, n2z = np.where(swap, n2z, n1z), np.where(swap, n1z, n2z)
        dx, dy, dz = np.where(swap, -dx, dx), np.where(swap, -dy, dy), np.where(swap, -dz, dz)
        vx, vy, vz = _cross(dx, dy, dz, n1x, n1y, n1z)
        vn = np.sqrt((vx * vx + vy * vy) + vz * vz)
        vx, vy, vz = vx / vn, vy / vn, vz / vn
        wx, wy, wz = _cross(n1x, n1y, n1z, vx, vy, vz)
        f2 = _dot(vx, vy, vz, n2x, n2y, n2z)
        f1 = np.arctan2(_dot(wx, wy, wz, n2x, n2y, n2z), _dot(n1x, n1y, n1z, n2x, n2y, n2z))
        scaled = np.stack([11.0 * ((f1 + PI) * INV_TWO_PI), 11.0 * ((f2 + 1.0) * 0.5), 11.0 * ((f3 + 1.0) * 0.5)], axis=-1)
        valid = (f4 != 0.0) & (vn != 0.0) & np.isfinite(ni).all(axis=-1) & np.isfinite(nj).all(axis=-1)
        valid &= ~np.isnan(f4) & ~np.isnan(vn)
    return scaled, valid


def bins_of(scaled):
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmax(np.floor(scaled), 0.0), float(BINS - 1)).astype(np.int64)


def margins_of(scaled):
    """(...) float64: the distance of the three scaled features to the nearest edge that separates two bins."""
    edges = np.arange(1, BINS, dtype=np.float64)
    m = np.abs(scaled[..., None] - edges).min(axis=-1)                       # interior edges, all three features
    m1 = np.minimum(np.abs(scaled[..., 0]), np.abs(scaled[..., 0] - float(BINS)))   # f1: the wrap at +-pi
    return np.minimum(m.min(axis=-1), m1)


def count_table(k):
    """tab[c] = 0.0f + hist_incr, c times, in float32."""
    incr = np.float32(100.0) / np.float32(k - 1)
    tab = np.zeros(64, np.float32)
    acc = np.float32(0.0)
    for c in range(1, 64):
        acc = np.float32(acc + incr)
        tab[c] = acc
    return tab


class Fpfh:
    """idx, d2 (n, k); counts (n, 33) int; spfh, fpfh (n, 33) float32; margin (n, k) float64 (inf for a skipped pair); valid (n, k):
    the pairs that were counted; fragile (n,): a pair below FRAGILE_BELOW; fragile_nb (n,): fragile, or a fragile record among the
    neighbours; nan_rows (n,): the records that get NaNs."""


def fpfh(xyz, normals, k, knn_result=None):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(np.asarray(normals, np.float32)[:, :3])
    n = len(xyz)
    if not 2 <= k <= 64:
        raise ValueError("k must be between 2 and 64")
    if len(nrm) != n:
        raise ValueError("one normal per record")
    r = Fpfh()
    r.idx, r.d2 = knn_result if knn_result is not None else N.knn(xyz, k)
    fin = r.idx[:, 0] >= 0
    own = np.arange(n)[:, None]
    j = np.where(r.idx >= 0, r.idx, 0)
    scaled, valid = pair_features(xyz[:, None, :], nrm[:, None, :], xyz[j], nrm[j])
    valid = valid & fin[:, None] & (j != own)
    r.valid = valid
    r.scaled = scaled
    r.margin = np.where(valid, margins_of(scaled), np.inf)
    b = bins_of(scaled) + np.arange(3) * BINS                                # (n, k, 3): places in the row
    flat = (own[:, :, None] * ROW + b)[valid]
    r.counts = np.bincount(flat.reshape(-1), minlength=n * ROW).reshape(n, ROW)
    r.spfh = count_table(k)[r.counts]
    r.nan_rows = ~fin | ~np.isfinite(nrm).all(axis=1)

    # the weighting, float32 throughout, in PCL's order
    h = np.zeros((n, ROW), np.float32)
    sums = np.zeros((n, 3), np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a in range(k):
            skip = (r.d2[:, a] == 0) | ~fin
            w = (np.float32(1.0) / r.d2[:, a]).astype(np.float32)
            val = (r.spfh[j[:, a]] * w[:, None]).astype(np.float32)
            h = np.where(skip[:, None], h, (h + val).astype(np.float32))
            for t in range(3):
                s = sums[:, t]
                for bb in range(BINS):
                    s = np.where(skip, s, (s + val[:, t * BINS + bb]).astype(np.float32))
                sums[:, t] = s
        scale = np.where(sums != 0, (100.0 / sums.astype(np.float64)).astype(np.float32), sums)
        out = (h.reshape(n, 3, BINS) * scale[:, :, None]).astype(np.float32).reshape(n, ROW)
    out[r.nan_rows] = np.nan
    r.fpfh = out
    r.fragile = (r.margin < FRAGILE_BELOW).any(axis=1)
    r.fragile_nb = r.fragile | (r.fragile[j] & fin[:, None]).any(axis=1)
    return r


def blocks_ok(rows, tol=1e-3):
    """Every block of 11 bins of every row sums to 100 within tol, or is all zero."""
    b = np.asarray(rows, np.float64).reshape(len(rows), 3, BINS)
    s = b.sum(axis=2)
    return (np.abs(s - 100.0) <= tol) | (b == 0).all(axis=2)
