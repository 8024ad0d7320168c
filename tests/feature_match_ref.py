"""The contract of feature matching (include/rsreg.h, "feature matching") in numpy: the yardstick of tests/test_feature_match_gpu.py.

Descriptor rows are (n, 33) float32.  A row is valid when all 33 floats are finite.  d2 is FLANN's L2_Simple<float>: a loop over the
33 bins on whole (ns, nt) float32 arrays, so every `+=` is ONE rounded float32 addition and every product one rounded float32
multiplication, in the contract's order -- numpy's element-wise ufuncs fuse nothing.  Selection is np.lexsort on (index, d2); the
correspondence rules are plain Python with the float-to-double compare spelled out.
"""
import numpy as np

DIM = 33
DBL_MAX = float(np.finfo(np.float64).max)


def valid_rows(rows):
    return np.isfinite(np.asarray(rows, np.float32)[:, :DIM]).all(axis=1)


def d2_matrix(src, tgt):
    """(ns, nt) float32: d2 = 0.0f; for b in 0 .. 32: diff = s[b] - t[b]; d2 += diff * diff.  Rows that are not valid give whatever
    the arithmetic gives (NaN, inf): the callers never look at them."""
    src, tgt = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    d2 = np.zeros((len(src), len(tgt)), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(DIM):
            diff = src[:, b, None] - tgt[None, :, b]
            assert diff.dtype == np.float32
            d2 += diff * diff
    return d2


def knn_from_d2(d2, src_valid, tgt_valid, k):
    """The k valid target rows with the smallest d2 for every valid source row, ascending by (d2, target index): (index (ns, k)
    int32, sqr_dist (ns, k) float32); a source row that is not valid gets -1 and 0.  Fewer than k valid target rows: ValueError (the
    library refuses the call)."""
    ns = len(src_valid)
    tv = np.flatnonzero(tgt_valid)
    if len(tv) < k:
        raise ValueError("fewer than k valid target rows")
    idx = np.full((ns, k), -1, np.int32)
    out = np.zeros((ns, k), np.float32)
    sv = np.flatnonzero(src_valid)
    if len(sv) == 0:
        return idx, out
    sub = d2[np.ix_(sv, tv)]
    assert not np.isnan(sub).any()                      # valid rows: squares and their sums, +inf at most
    cols = np.broadcast_to(tv[None, :], sub.shape)
    order = np.lexsort((cols, sub), axis=-1)[:, :k]     # primary key d2, then the target index
    idx[sv] = np.take_along_axis(cols, order, axis=1).astype(np.int32)
    out[sv] = np.take_along_axis(sub, order, axis=1)
    return idx, out


def knn(src, tgt, k):
    return knn_from_d2(d2_matrix(src, tgt), valid_rows(src), valid_rows(tgt), k)


def correspondences_from_d2(d2, src_valid, tgt_valid, max_distance=DBL_MAX, reciprocal=False):
    """pcl::registration::CorrespondenceEstimation::determineCorrespondences / determineReciprocalCorrespondences as the header
    recalls them: a list of (index_query, index_match, distance) with distance the float32 squared distance."""
    max_distance = float(max_distance)
    max_dist_sqr = max_distance * max_distance          # in double; DBL_MAX * DBL_MAX is +inf
    out = []
    if not tgt_valid.any() or not src_valid.any():
        return out
    fwd_i, fwd_d = knn_from_d2(d2, src_valid, tgt_valid, 1)
    if reciprocal:
        rev_i, rev_d = knn_from_d2(d2.T, tgt_valid, src_valid, 1)
    for i in range(len(src_valid)):
        if not src_valid[i]:
            continue
        j, dist = int(fwd_i[i, 0]), fwd_d[i, 0]
        if float(np.float64(dist)) > max_dist_sqr:      # (double)d2 > max_dist_sqr: a distance AT the bound is kept
            continue
        if reciprocal:
            back, back_d = int(rev_i[j, 0]), rev_d[j, 0]
            if float(np.float64(back_d)) > max_dist_sqr or back != i:
                continue
        out.append((i, j, dist))
    return out


def correspondences(src, tgt, max_distance=DBL_MAX, reciprocal=False):
    return correspondences_from_d2(d2_matrix(src, tgt), valid_rows(src), valid_rows(tgt), max_distance, reciprocal)


CORRESPONDENCE_DTYPE = np.dtype([("index_query", np.int32), ("index_match", np.int32), ("distance", np.float32)])


def as_records(pairs):
    """The list of correspondences() as the 12-byte records the library writes."""
    rec = np.zeros(len(pairs), CORRESPONDENCE_DTYPE)
    for n, (i, j, dist) in enumerate(pairs):
        rec[n] = (i, j, dist)
    return rec
