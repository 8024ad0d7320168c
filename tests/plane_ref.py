"""A reference of point-to-plane ICP as include/rsreg.h defines it (RSREG_NUM_PLANE_SUMS, rsreg_plane_solve_from_sums),
numpy only, independent of the engine:

  * a kept pair: p = the transformed source point, q = its matched target point, n = that target record's normal (float32),
    W = its weight; in float64 from the float32 inputs, one rounding per operation:
        a = p x n,  J = [a0 a1 a2 nx ny nz],  r = ((nx*qx + ny*qy) + nz*qz) - ((nx*px + ny*py) + nz*pz)
        terms W * (J_i * J_j), W * (J_i * r), W * (r * r), W * d2
    so every TERM equals the engine's bit for bit and only the order of the additions differs;
  * plane_sums returns the 32 sums and, per sum, sum|term| and the number of terms: a sum of N terms, however ordered, is
    within (N + 16) * 2^-53 * sum|term| of the exact one (N - 1 roundings, each at most 2^-53 of a partial sum that is at
    most sum|term|; the + 16 leaves room for second-order terms);
  * plane_solve: numpy.linalg.eigh of AtA, the pseudo-inverse over the eigenvalues above ([2] + 80) * 2^-53 * trace(AtA),
    T = Rz(gamma) Ry(beta) Rx(alpha), t = (tx, ty, tz) (PCL's constructTransformationMatrix), rounded to float32;
  * plane_icp: the whole loop -- float32 nearest neighbour (fitness_ref.d2_f32, ties to the lowest index), the gate
    `not (double(d2) > gate^2)`, sums, solve, final = T_inc * final in float32 ((a0 b0 + a1 b1) + a2 b2) + a3 b3, the source
    moved by T_inc in float32 (filters_ref.transform).  Up to 2^24 source x target pairs the search is a chunked brute force;
    beyond, filters_ref.nearest: the same float32 distances and the same tie rule over cKDTree candidates.
"""
import math

import numpy as np

import filters_ref
from fitness_ref import d2_f32, finite_rows

NUM_PLANE_SUMS = 32
U = 2.0 ** -53
_BRUTE = 1 << 24


def pair_terms(p, q, n, w, d2):
    """(m, 32) float64 terms of m pairs (rows of float32 p, q, n; weights w; float32 d2), and which pairs enter the system."""
    p = np.asarray(p, np.float32).astype(np.float64)
    q = np.asarray(q, np.float32).astype(np.float64)
    nf = np.asarray(n, np.float32)
    ok = np.isfinite(nf).all(axis=1)
    n = np.where(ok[:, None], nf, np.float32(0)).astype(np.float64)
    W = np.asarray(w, np.float64)
    px, py, pz = p.T
    qx, qy, qz = q.T
    nx, ny, nz = n.T
    J = np.stack([nz * py - ny * pz, nx * pz - nz * px, ny * px - nx * py, nx, ny, nz], axis=1)
    r = ((nx * qx + ny * qy) + nz * qz) - ((nx * px + ny * py) + nz * pz)
    t = np.zeros((len(p), NUM_PLANE_SUMS))
    t[:, 0] = W
    t[:, 1] = W * np.asarray(d2, np.float32).astype(np.float64)
    t[:, 2] = W
    t[:, 3] = W * (r * r)
    k = 4
    for i in range(6):
        for j in range(i, 6):
            t[:, k] = W * (J[:, i] * J[:, j])
            k += 1
    for i in range(6):
        t[:, 25 + i] = W * (J[:, i] * r)
    t[~ok, 2:] = 0.0
    return t, ok


def plane_sums(p, q, n, w, d2=None):
    """(sums, sum|term| per sum, terms per sum) over the given pairs."""
    if d2 is None:
        d2 = d2_f32(np.asarray(p, np.float32), np.asarray(q, np.float32))
    t, ok = pair_terms(p, q, n, w, d2)
    sums = t.sum(axis=0)
    mag = np.abs(t).sum(axis=0)
    cnt = np.full(NUM_PLANE_SUMS, float(len(t)))
    cnt[2:] = float(ok.sum())
    return sums, mag, cnt


def sums_bound(mag, cnt):
    return (cnt + 16.0) * U * mag


def system(sums):
    A = np.zeros((6, 6))
    k = 4
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = sums[k]
            k += 1
    return A, np.asarray(sums[25:31], np.float64)


def rank_cut(sums):
    A, _ = system(sums)
    return (sums[2] + 80.0) * U * np.trace(A)


def euler_matrix(x):
    a, b, g = (float(v) for v in x[:3])
    sa, ca, sb, cb, sg, cg = math.sin(a), math.cos(a), math.sin(b), math.cos(b), math.sin(g), math.cos(g)
    T = np.eye(4)
    T[:3, :3] = [[cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca],
                 [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca],
                 [-sb, cb * sa, cb * ca]]
    T[:3, 3] = x[3:6]
    return T.astype(np.float32)


def plane_solve(sums, want_x=False):
    """(T float32 4x4, rank[, x]) of the 32 sums."""
    sums = np.asarray(sums, np.float64)
    x = np.zeros(6)
    rank = 0
    if sums[2] > 0:
        A, b = system(sums)
        w, v = np.linalg.eigh(A)
        cut = rank_cut(sums)
        for e in range(5, -1, -1):
            if w[e] > cut:
                x += v[:, e] * ((v[:, e] @ b) / w[e])
                rank += 1
        if not np.isfinite(x).all():
            x[:] = 0
            rank = 0
    T = euler_matrix(x) if rank else np.eye(4, dtype=np.float32)
    return (T, rank, x) if want_x else (T, rank)


def mul_f32(a, b):
    """c = a * b in float32, ((a0 b0 + a1 b1) + a2 b2) + a3 b3 (host_linalg.hpp: mul)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    c = np.empty((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            c[i, j] = ((a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]) + a[i, 3] * b[3, j]
    return c


def nearest_brute(q, t, chunk=256):
    """float32 nearest finite target of every finite query: (index or -1, float32 d2), ties to the lowest index."""
    q = np.ascontiguousarray(q, np.float32)
    t = np.ascontiguousarray(t, np.float32)
    tf = np.flatnonzero(finite_rows(t))
    idx = np.full(len(q), -1, np.int64)
    d2 = np.zeros(len(q), np.float32)
    rows = np.flatnonzero(finite_rows(q))
    if not len(tf):
        return idx, d2
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, len(rows), chunk):
            r = rows[s:s + chunk]
            d = d2_f32(q[r, None, :], t[None, tf, :])
            a = d.argmin(axis=1)   # (the first minimum: the lowest index)
            idx[r] = tf[a]
            d2[r] = d[np.arange(len(r)), a]
    return idx, d2


def nearest(q, t, gate):
    if len(q) * len(t) <= _BRUTE:
        return nearest_brute(q, t)
    g = float(gate)
    bound = g * (1 + 1e-5) + 1e-12 if g < 1e18 else np.inf
    return filters_ref.nearest(q, t, bound)


class PlaneIcp:
    """T (float32 4x4), iterations, n_correspondences and sums of the last iteration, state ('ITERATIONS' or
    'NO_CORRESPONDENCES'), errors (per iteration |final - truth|_F when `truth` is given)."""


def plane_icp(src, tgt, normals, guess=None, max_iterations=10, gate=0.05, truth=None, point_to_plane=True):
    """RSREG_CRITERIA_FIXED: exactly max_iterations iterations unless fewer than 3 pairs are left.  src, tgt: (n, 3) float32
    records (non-finite ones never match); normals: (n_tgt, 3) float32.  point_to_plane=False: the same loop with the
    point-to-point solve (Umeyama over the kept pairs in float64), for comparison on the same matches."""
    s = np.ascontiguousarray(src, np.float32)
    t = np.ascontiguousarray(tgt, np.float32)
    nrm = np.ascontiguousarray(normals, np.float32)
    final = np.eye(4, dtype=np.float32) if guess is None else np.asarray(guess, np.float32).copy()
    cur = s.copy()
    fin = finite_rows(s)
    cur[fin] = filters_ref.transform(s[fin], None if guess is None else final)
    gate2 = float(gate) * float(gate)
    r = PlaneIcp()
    r.iterations, r.state, r.errors, r.sums, r.n_correspondences = 0, "ITERATIONS", [], None, 0
    for _ in range(max_iterations):
        idx, d2 = nearest(cur, t, gate)
        keep = (idx >= 0) & ~(d2.astype(np.float64) > gate2)
        k = np.flatnonzero(keep)
        sums, _, _ = plane_sums(cur[k], t[idx[k]], nrm[idx[k]], np.ones(len(k)), d2[k])
        r.sums, r.n_correspondences = sums, int(len(k))
        if len(k) < 3:
            r.state = "NO_CORRESPONDENCES"
            break
        T_inc = plane_solve(sums)[0] if point_to_plane else umeyama(cur[k], t[idx[k]])
        final = mul_f32(T_inc, final)
        cur[fin] = filters_ref.transform(cur[fin], T_inc)
        r.iterations += 1
        if truth is not None:
            r.errors.append(float(np.linalg.norm(final.astype(np.float64) - truth)))
    r.T = final
    return r


def umeyama(p, q):
    """Eigen::umeyama without scaling over the pairs, float64, rounded to float32 (the comparison loop only)."""
    p, q = p.astype(np.float64), q.astype(np.float64)
    mp, mq = p.mean(0), q.mean(0)
    S = (q - mq).T @ (p - mp) / len(p)
    Uu, _, Vt = np.linalg.svd(S)
    D = np.eye(3)
    if np.linalg.det(Uu) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1
    R = Uu @ D @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mq - R @ mp
    return T.astype(np.float32)
