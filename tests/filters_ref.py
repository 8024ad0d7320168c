"""A reference of the ICP correspondence filters that scales to whole frames (10^6 points), independent of the
engine and of the oracle's C code: cKDTree candidates, rescored in float32 in FLANN's order, every tie closed exactly.

Spec (rsreg.h, oracle/icp_oracle.c):
  * nearest target of every finite source record, d2 = ((dx*dx + dy*dy) + dz*dz) in float32, lowest index among ties;
  * gate: the pair is kept unless double(d2) > gate * gate;
  * reciprocal: the pair (i, t) is kept only if i is the nearest finite source record of target t (lowest index among ties);
  * trimmed rejector (0 < ratio < 1): of the `count` remaining pairs the first int(floorf(float(ratio) * float(count))) in
    the order (d2, source index) are kept;
  * non-finite records never match.
"""
import numpy as np
from scipy.spatial import cKDTree

_K0 = 8          # candidates asked of the tree first; rows whose ties are not closed by them ask for 4x as many
_REL = 1e-5      # float32 rescoring can reorder float64 distances by a few ulp: candidates this close are all rescored


def xyz(cloud):
    """(n, 3) float32 of a PointCloud, a structured array or an (n, >=3) float32 array."""
    a = getattr(cloud, "points", cloud)
    a = np.asarray(a)
    if a.dtype.names:
        return np.stack([a["x"], a["y"], a["z"]], axis=1).astype(np.float32)
    return np.ascontiguousarray(a[:, :3], np.float32)


def transform(pts, T):
    """PCL transformCloud in float32: x' = ((m00*x + m01*y) + m02*z) + m03 (no fused operations)."""
    if T is None:
        return pts.copy()
    T = np.asarray(T, np.float32)
    out = np.empty_like(pts)
    for r in range(3):
        out[:, r] = ((T[r, 0] * pts[:, 0] + T[r, 1] * pts[:, 1]) + T[r, 2] * pts[:, 2]) + T[r, 3]
    return out


def d2_f32(a, b):
    """FLANN L2_Simple<float>: ((dx*dx + dy*dy) + dz*dz), every step rounded to float32."""
    dx, dy, dz = (np.subtract(a[..., k], b[..., k], dtype=np.float32) for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def _distinct(a):
    """Rows of a finite (n, 3) float32 array without copies: (distinct rows, lowest index of each, row -> distinct row)."""
    u, first, inv = np.unique(a, axis=0, return_index=True, return_inverse=True)
    return u, first, inv.reshape(-1)


def nearest(queries, points, bound=np.inf):
    """Nearest finite point of every finite query: (index, float32 d2); -1 where there is none (within `bound`, a
    float64 Euclidean distance the caller's gate fits in).  Ties on the float32 d2: the lowest index."""
    q = np.asarray(queries, np.float32)
    p = np.asarray(points, np.float32)
    idx = np.full(len(q), -1, np.int64)
    dist = np.zeros(len(q), np.float32)
    qf = np.nonzero(np.isfinite(q).all(1))[0]
    pf = np.nonzero(np.isfinite(p).all(1))[0]
    if not len(qf) or not len(pf):
        return idx, dist
    # copies of a point tie exactly: the lowest index stands for them all; copies of a query get the same answer
    pu, p_first, _ = _distinct(p[pf])
    p_low = pf[p_first]
    qu, _, q_inv = _distinct(q[qf])
    tree = cKDTree(pu.astype(np.float64))
    qd = qu.astype(np.float64)
    best = np.full(len(qu), np.inf, np.float32)
    arg = np.full(len(qu), -1, np.int64)
    todo = np.arange(len(qu))
    k = min(_K0, len(pu))
    while len(todo):
        dd, ii = tree.query(qd[todo], k=k, distance_upper_bound=bound)
        dd, ii = dd.reshape(len(todo), k), ii.reshape(len(todo), k)
        have = ii < len(pu)
        cand = p_low[np.where(have, ii, 0)]
        sc = np.where(have, d2_f32(qu[todo][:, None, :], p[cand]), np.float32(np.inf))
        b = sc.min(1)
        a = np.where(have & (sc == b[:, None]), cand, np.iinfo(np.int64).max).min(1)
        # closed: fewer than k points within the bound (all of them are here), or the k-th lies clearly beyond the best
        closed = ~have[:, -1] | (dd[:, -1] ** 2 > b.astype(np.float64) * (1 + _REL) + 1e-30) | (k >= len(pu))
        best[todo[closed]] = b[closed]
        arg[todo[closed]] = np.where(have[closed, 0], a[closed], -1)
        todo = todo[~closed]
        k = min(4 * k, len(pu))   # equidistant neighbours (lattices): ask for more until the ties are closed
    found = arg[q_inv] >= 0
    idx[qf[found]] = arg[q_inv][found]
    dist[qf[found]] = best[q_inv][found]
    return idx, dist


def trim_keep(ratio, count):
    """CorrespondenceRejectorTrimmed: int(floor(overlap_ratio * float(size))), in float like PCL."""
    return int(np.floor(np.float32(ratio) * np.float32(count)))


def search(src, tgt, gate, reciprocal=False, ratio=0.0, guess=None):
    """One correspondence search with the filters: (index per source record or -1, float32 d2 of its nearest target
    point (0 where there is none), the pairs before the trim, the number kept)."""
    s = transform(xyz(src), guess)
    t = xyz(tgt)
    gate2 = float(gate) * float(gate)
    bound = np.sqrt(gate2) * (1 + _REL) + 1e-12
    idx, dist = nearest(s, t, bound)
    ok = (idx >= 0) & ~(dist.astype(np.float64) > gate2)
    if reciprocal:
        cand = np.nonzero(ok)[0]
        tu, inv = np.unique(idx[cand], return_inverse=True)
        back, _ = nearest(t[tu], s, bound)
        ok[cand[back[inv] != cand]] = False
    count = int(ok.sum())
    if 0 < ratio < 1:
        keep = trim_keep(ratio, count)
        if keep < count:
            cand = np.nonzero(ok)[0]
            order = cand[np.lexsort((cand, dist[cand]))]
            ok[order[keep:]] = False
    return np.where(ok, idx, -1).astype(np.int32), dist, count


def sums(src, tgt, index, d2, guess=None):
    """The 17 sums of the kept pairs in float64: count, sum p, sum q, sum q p^T (row-major), sum d2."""
    s = transform(xyz(src), guess).astype(np.float64)
    t = xyz(tgt).astype(np.float64)
    m = index >= 0
    P, Q = s[m], t[index[m]]
    out = np.zeros(17)
    out[0] = m.sum()
    out[1:4] = P.sum(0)
    out[4:7] = Q.sum(0)
    out[7:16] = np.einsum("nr,nc->rc", Q, P).reshape(9)
    out[16] = d2[m].astype(np.float64).sum()
    return out


def cut_block(index, d2, pre_count, ratio, pre_index):
    """How the trim's cut meets the pairs at its distance: (tied pairs before the cut, tied pairs after it).  A case whose
    cut falls inside a block of equal distances has both > 0.  pre_index: the matches before the trim."""
    keep = trim_keep(ratio, pre_count)
    if not (0 < ratio < 1) or keep >= pre_count or keep == 0:
        return 0, 0
    cand = np.nonzero(pre_index >= 0)[0]
    order = cand[np.lexsort((cand, d2[cand]))]
    cut = d2[order[keep - 1]]
    return int((d2[order[:keep]] == cut).sum()), int((d2[order[keep:]] == cut).sum())
