"""A reference of the exact k-nearest-neighbour search with indices (rsreg_cloud_knn) and of pcl::NormalEstimation with
setKSearch as include/rsreg.h defines it (rsreg_cloud_normals), numpy only (scipy's cKDTree for the large clouds), independent of
the engine:

  * the search runs over the finite records only; for every finite record the float32 squared distances
    ((dx*dx + dy*dy) + dz*dz, fitness_ref.d2_f32) to all of them, itself and exact copies included, chunked brute force;
    np.lexsort by (d2, original record index), the first k.  A non-finite record's row is all -1 / all 0;
  * d = neighbour - record in float64, C = (sum d d^T) / k - (sum d / k)(sum d / k)^T, np.linalg.eigh;
  * normal = the eigenvector of the smallest eigenvalue l0; curvature = float32(|l0 / (l0 + l1 + l2)|), 0 when the trace is 0;
    all neighbours in one place (trace 0): (0, 0, 1), curvature 0;
  * flipped when, with v = viewpoint - record in float32, (v.x * nx + v.y * ny) + v.z * nz < 0 in float32 on the float32 normal;
  * a non-finite record gets NaNs.

Beyond 2^26 pairs the brute force is replaced by cKDTree candidates rescored and ordered the same way: a row is closed once its
last float64 candidate lies clearly beyond its k-th float32 value, so that every record that ties with the k-th value is among the
candidates.  tests/test_normals_cpu.py holds the two paths against each other.
"""
import numpy as np

from fitness_ref import d2_f32, finite_rows

_BRUTE = 1 << 26   # query x point pairs the chunked brute force takes; beyond: the tree


def _check(n_fin, k):
    if k < 1:
        raise ValueError("k must be at least 1")
    if n_fin < k:
        raise ValueError("fewer than k finite records")


def _first_k(d, cand, k):
    """d: (rows, m) float32 distances, cand: (rows, m) or (m,) original indices -> the first k by (d2, index)."""
    cand = np.broadcast_to(cand, d.shape)
    # (only the records not beyond the k-th value can be among the first k: the lexsort runs over those)
    kth = np.partition(d, k - 1, axis=1)[:, k - 1:k]
    m = int((d <= kth).sum(axis=1).max())
    if m < d.shape[1]:
        part = np.argpartition(d, m - 1, axis=1)[:, :m]
        d, cand = np.take_along_axis(d, part, 1), np.take_along_axis(cand, part, 1)
    order = np.lexsort((cand, d), axis=1)[:, :k]
    return np.take_along_axis(cand, order, 1), np.take_along_axis(d, order, 1)


def knn_brute(q, t, orig, k, chunk=128):
    """The first k of the points t (original indices orig) for every query of q."""
    idx = np.empty((len(q), k), np.int64)
    d2 = np.empty((len(q), k), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, len(q), chunk):
            d = d2_f32(q[s:s + chunk, None, :], t[None, :, :])
            idx[s:s + chunk], d2[s:s + chunk] = _first_k(d, orig, k)
    return idx, d2


def knn_tree(q, t, orig, k, workers=-1):
    from scipy.spatial import cKDTree
    idx = np.empty((len(q), k), np.int64)
    d2 = np.empty((len(q), k), np.float32)
    todo = np.arange(len(q))
    q64 = q.astype(np.float64)
    tree = cKDTree(t.astype(np.float64))
    kc = min(2 * k + 8, len(t))
    while len(todo):
        dist, ci = tree.query(q64[todo], kc, workers=workers)
        dist, ci = dist.reshape(len(todo), -1), ci.reshape(len(todo), -1)
        ri = np.empty((len(todo), k), np.int64)
        rd = np.empty((len(todo), k), np.float32)
        step = max(1, (1 << 22) // kc)
        with np.errstate(over="ignore", invalid="ignore"):
            for s in range(0, len(todo), step):
                rows = slice(s, s + step)
                d = d2_f32(q[todo[rows]][:, None, :], t[ci[rows]])
                ri[rows], rd[rows] = _first_k(d, orig[ci[rows]], k)
        kth = rd[:, -1].astype(np.float64)
        closed = (kc >= len(t)) | (dist[:, -1] ** 2 > kth * (1 + 1e-5) + 1e-30)   # (float32 rescoring moves a d2 by a few ulp)
        idx[todo[closed]], d2[todo[closed]] = ri[closed], rd[closed]
        todo = todo[~closed]
        kc = min(2 * kc, len(t))
    return idx, d2


def knn(xyz, k, method=None):
    """(idx (n, k) int32, d2 (n, k) float32): ascending by (d2, original index); a non-finite record's row is -1 / 0."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    fin = finite_rows(xyz)
    orig = np.flatnonzero(fin)
    t = xyz[fin]
    _check(len(t), k)
    if method is None:
        method = "brute" if len(t) * len(t) <= _BRUTE else "tree"
    q, inv = np.unique(t, axis=0, return_inverse=True)   # (exact copies ask the same question: it is answered once)
    inv = inv.reshape(-1)
    fi, fd = knn_brute(q, t, orig, k) if method == "brute" else knn_tree(q, t, orig, k)
    idx = np.full((len(xyz), k), -1, np.int32)
    d2 = np.zeros((len(xyz), k), np.float32)
    idx[fin], d2[fin] = fi[inv], fd[inv]
    return idx, d2


def covariances(xyz, idx):
    """(C (n, 3, 3), finite mask): float64 covariance of every finite record's neighbours about the record itself."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    fin = idx[:, 0] >= 0
    k = idx.shape[1]
    p = xyz.astype(np.float64)
    C = np.zeros((len(xyz), 3, 3))
    rows = np.flatnonzero(fin)
    for s in range(0, len(rows), 1 << 16):
        r = rows[s:s + (1 << 16)]
        d = p[idx[r]] - p[r][:, None, :]
        m = d.sum(axis=1) / k
        C[r] = np.einsum("nki,nkj->nij", d, d) / k - m[:, :, None] * m[:, None, :]
    return C, fin


def cos_view(xyz, normal, viewpoint=(0.0, 0.0, 0.0)):
    """PCL's flipNormalTowardsViewpoint in its float arithmetic: (v.x * nx + v.y * ny) + v.z * nz, v = viewpoint - p."""
    v = (np.asarray(viewpoint, np.float32)[None, :] - np.asarray(xyz, np.float32)).astype(np.float32)
    n = np.asarray(normal, np.float32)
    with np.errstate(invalid="ignore"):
        return ((v[:, 0] * n[:, 0] + v[:, 1] * n[:, 1]).astype(np.float32) + v[:, 2] * n[:, 2]).astype(np.float32)


def gap_ratio(evals):
    """(l1 - l0) / l2 (0 where l2 is 0): how well the data fixes the direction of the normal."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(evals[:, 2] > 0, (evals[:, 1] - evals[:, 0]) / evals[:, 2], 0.0)


class Normals:
    """Everything the checks read: idx, d2, C, evals (ascending), normal (float32, flipped), curvature (float32), cos
    (the float32 cos_view of the UNFLIPPED float32 eigenvector), finite, trace."""


def normals(xyz, k, viewpoint=(0.0, 0.0, 0.0), knn_result=None):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    r = Normals()
    r.idx, r.d2 = knn_result if knn_result is not None else knn(xyz, k)
    r.C, r.finite = covariances(xyz, r.idx)
    r.trace = np.trace(r.C, axis1=1, axis2=2)
    w, v = np.linalg.eigh(r.C)
    r.evals = w
    n = v[:, :, 0].copy()
    flat = r.trace == 0
    n[flat] = (0.0, 0.0, 1.0)
    s = w.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = np.where((r.trace == 0) | (s == 0), 0.0, np.abs(w[:, 0] / s))
    n32 = n.astype(np.float32)
    r.cos = cos_view(xyz, n32, viewpoint)
    with np.errstate(invalid="ignore"):
        n32[r.cos < 0] *= np.float32(-1)
    r.normal = n32
    r.curvature = curv.astype(np.float32)
    r.normal[~r.finite] = np.nan
    r.curvature[~r.finite] = np.nan
    r.gap = gap_ratio(w)
    return r
