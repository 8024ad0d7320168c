"""A reference of pcl::PassThrough and pcl::StatisticalOutlierRemoval (PCL 1.9.1, recalled; unorganized input, kd-tree search),
independent of the engine:

  * the tree holds the finite records only; a non-finite record has distance 0 and is not "valid" (kept unless `negative`);
  * for each finite record the mean_k + 1 smallest float32 squared distances ((dx*dx + dy*dy) + dz*dz, FLANN L2_Simple<float>)
    to the tree's points, itself and copies included -- chunked brute force up to 2^25 pairs, beyond that cKDTree candidates
    rescored in float32, a row widened until its last float64 candidate lies clearly beyond its (k + 1)-th float32 value;
  * sorted ascending, the first (the point itself) dropped, dist_sum = sum of (double) sqrtf(d2[j]) one after the other,
    distance = (float)(dist_sum / mean_k);
  * over all records in input order: sum += d, sq += d * d in double; mean = sum / n_valid,
    var = (sq - sum * sum / n_valid) / (n_valid - 1), threshold = mean + stddev_mult * sqrt(var);
  * removed when distance > threshold (negative: when distance <= threshold); kept records keep their order.

Equal distances are equal values, so the order among ties never enters a result.
"""
import numpy as np
from scipy.spatial import cKDTree

from fitness_ref import d2_f32, finite_rows

_BRUTE = 1 << 25   # query x point pairs the chunked brute force takes; beyond: the tree
FLT_MIN, FLT_MAX = np.finfo(np.float32).tiny, np.finfo(np.float32).max


def _check(n_fin, mean_k):
    if mean_k < 1:
        raise ValueError("mean_k must be at least 1")
    if n_fin < mean_k + 1:
        raise ValueError("fewer than mean_k + 1 finite records (PCL reads past its arrays)")


def _mean_of_sorted(d2, mean_k):
    """d2: (rows, mean_k + 1) float32, ascending -> float32 mean distances."""
    root = np.sqrt(d2[:, 1:].astype(np.float32)).astype(np.float64)   # float sqrt, then double
    dist_sum = np.cumsum(root, axis=1)[:, -1]                          # added one after the other, ascending
    return (dist_sum / float(mean_k)).astype(np.float32)


def smallest_d2_brute(t, k1, chunk=128):
    """The k1 smallest float32 squared distances of every row of t (finite, float32) to the rows of t, ascending."""
    out = np.empty((len(t), k1), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, len(t), chunk):
            d = d2_f32(t[s:s + chunk, None, :], t[None, :, :])
            out[s:s + chunk] = np.sort(np.partition(d, k1 - 1, axis=1)[:, :k1], axis=1)
    return out


def smallest_d2_tree(t, k1, workers=-1):
    """The same through cKDTree candidates rescored in float32.  A row is closed once every point outside its candidate list
    is clearly farther (in float64) than its k1-th float32 value -- float32 rescoring moves a squared distance by a few ulp at
    most -- or once that value is 0 (k1 copies of the query: nothing is smaller), or once the list holds every point."""
    out = np.empty((len(t), k1), np.float32)
    todo = np.arange(len(t))
    t64 = t.astype(np.float64)
    tree = cKDTree(t64)
    kc = min(2 * k1, len(t))
    while len(todo):
        dist, idx = tree.query(t64[todo], kc, workers=workers)
        dist, idx = dist.reshape(len(todo), -1), idx.reshape(len(todo), -1)
        d = np.empty((len(todo), k1), np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            for s in range(0, len(todo), 65536):   # (the rescoring's temporaries: rows x candidates x 3 floats)
                rows = slice(s, s + 65536)
                d[rows] = np.sort(d2_f32(t[todo[rows]][:, None, :], t[idx[rows]]), axis=1)[:, :k1]
        kth = d[:, -1].astype(np.float64)
        closed = (kc >= len(t)) | (kth == 0.0) | (dist[:, -1] ** 2 > kth * (1 + 1e-5) + 1e-30)
        out[todo[closed]] = d[closed]
        todo = todo[~closed]
        kc = min(2 * kc, len(t))
    return out


def knn_mean_distance(xyz, mean_k, method=None):
    """float32 distance of every record (0 for a non-finite one).  method: "brute", "tree" or None (by size)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    fin = finite_rows(xyz)
    t = xyz[fin]
    _check(len(t), mean_k)
    if method is None:
        method = "brute" if len(t) * len(t) <= _BRUTE else "tree"
    d2 = smallest_d2_brute(t, mean_k + 1) if method == "brute" else smallest_d2_tree(t, mean_k + 1)
    out = np.zeros(len(xyz), np.float32)
    out[fin] = _mean_of_sorted(d2, mean_k)
    return out


def sor_stats(xyz, dist, stddev_mult):
    """(n_valid, mean, stddev, threshold) the way PCL adds them up: every record's distance, divided by the valid ones."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n_valid = int(finite_rows(xyz).sum())
    if n_valid < 2:
        raise ValueError("fewer than two finite records (PCL divides by zero)")
    d = dist.astype(np.float64)
    s = float(np.cumsum(d)[-1])
    sq = float(np.cumsum(d * d)[-1])
    mean = s / n_valid
    var = (sq - s * s / n_valid) / (n_valid - 1)
    stddev = float(np.sqrt(var))
    return n_valid, mean, stddev, mean + stddev_mult * stddev


def sor_keep(xyz, dist, threshold, negative=False):
    """Which records stay, for a given threshold."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    fin = finite_rows(xyz)
    above = dist.astype(np.float64) > threshold
    keep = above if negative else ~above
    return np.where(fin, keep, not negative)


def sor(xyz, mean_k, stddev_mult, negative=False, method=None):
    """(keep mask, distances, (n_valid, mean, stddev, threshold))."""
    dist = knn_mean_distance(xyz, mean_k, method)
    stats = sor_stats(xyz, dist, stddev_mult)
    return sor_keep(xyz, dist, stats[3], negative), dist, stats


def threshold_margin(dist, xyz, threshold):
    """The smallest relative distance of a finite record's distance from the threshold."""
    fin = finite_rows(np.ascontiguousarray(xyz, np.float32).reshape(-1, 3))
    return float(np.min(np.abs(dist[fin].astype(np.float64) - threshold)) / abs(threshold))


def passthrough_keep(xyz, field, lo=FLT_MIN, hi=FLT_MAX, negative=False):
    """Which records pcl::PassThrough keeps: a non-finite record never; else v < lo || v > hi removes (negative: the others)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    v = xyz[:, field]
    with np.errstate(invalid="ignore"):
        outside = (v < np.float32(lo)) | (v > np.float32(hi))
    return finite_rows(xyz) & (outside if negative else ~outside)


def passthrough(points, field, lo=FLT_MIN, hi=FLT_MAX, negative=False, keep_organized=False):
    """The filtered records of a structured point array (fields x, y, z first), every byte of a record kept, and is_dense of the
    output (None: the input's)."""
    xyz = np.stack([points["x"], points["y"], points["z"]], axis=1)
    keep = passthrough_keep(xyz, field, lo, hi, negative)
    raw = np.ascontiguousarray(points).view(np.uint8).reshape(len(points), -1)   # (numpy's indexing of a padded record copies the fields only)
    if not keep_organized:
        return raw[keep].copy().view(points.dtype).reshape(-1), True
    out = raw.copy().view(points.dtype).reshape(-1)
    for f in ("x", "y", "z"):
        out[f][~keep] = np.float32(np.nan)
    return out, (None if keep.all() else False)
