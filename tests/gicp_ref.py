"""A reference of GeneralizedIterativeClosestPoint as include/rsreg.h defines it (the rsreg_gicp_* section), numpy only,
independent of the engine.  Every formula follows the header's operation order in float64, one rounding per operation (numpy
fuses nothing), so that C', M and a pair's 32 terms are reproducible term by term; only the order of the additions of a sum
differs from the engine's:

  * covariances: the neighbours' moments about the record and c = S / k - m m^T (normals_ref.covariances), n = the eigenvector of
    the smallest eigenvalue (numpy.linalg.eigh), (0, 0, 1) when the trace is 0, C'_ab = delta_ab - (1 - eps) * (n_a * n_b);
  * mahalanobis: B = R C_s, D = B R^T, A = C_t + D, the adjugate, det, M = adj * (1 / det); a pair with a non-finite covariance
    or a non-finite M is out of the system;
  * pair_terms / gicp_sums: the 32 terms of every pair at an increment X, their sums, sum|term| and number of terms;
  * step / delta / minimise: x = scale * pinv(H) b by plane_ref.plane_solve's rule, Delta(x) = Rz Ry Rx | t in double, the
    step control of the header driven by any `sums_at(X)` callable (the engine's too);
  * gicp: the whole loop -- the source under T in float32 (filters_ref.transform), plane_ref.nearest, the gate
    `not (double(d2) > gate^2)`, T_new = float32(X T), PCL's delta test.  perturb = (rng, rel): every evaluated sum is multiplied by
    1 + rel * u, u uniform in [-1, 1] -- the robustness probe of tests/test_gicp_cpu.py.
"""
import math

import numpy as np

import filters_ref
import normals_ref
import plane_ref
from fitness_ref import finite_rows

NUM_GICP_SUMS = 32
U = 2.0 ** -53
_UPPER = [(r, c) for r in range(3) for c in range(r, 3)]   # xx xy xz yy yz zz


class Params:
    def __init__(self, **kw):
        self.max_iterations, self.max_inner_iterations = 200, 20
        self.max_correspondence_distance = 5.0
        self.transformation_epsilon, self.rotation_epsilon = 5e-4, 2e-3
        self.k_correspondences, self.gicp_epsilon = 20, 1e-3
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


# ------------------------------------------------------------------------------------------------------------ covariances
def regularised(n, epsilon):
    """(m, 6) C' = I - (1 - epsilon) n n^T of unit vectors n (m, 3): the product, the scaling, the difference."""
    n = np.asarray(n, np.float64)
    s = 1.0 - float(epsilon)
    out = np.empty((len(n), 6))
    for k, (a, b) in enumerate(_UPPER):
        v = s * (n[:, a] * n[:, b])
        out[:, k] = (1.0 - v) if a == b else (0.0 - v)
    return out


def svd_rebuild(C, epsilon):
    """PCL's rule: the singular values of the covariance replaced by (1, 1, epsilon), U diag(1, 1, eps) U^T (3 x 3)."""
    Uu, _, _ = np.linalg.svd(C)
    return (Uu * np.array([1.0, 1.0, float(epsilon)])) @ Uu.T


class Cov:
    """cov (n, 6; NaN rows for non-finite records), normal (n, 3 float64), C (n, 3, 3), evals, gap, finite, idx"""


def covariances(xyz, k=20, epsilon=1e-3, idx=None):
    """The contract of rsreg_cloud_gicp_covariances; idx: the neighbour indices to use (the engine's own), else normals_ref.knn."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    r = Cov()
    r.idx = normals_ref.knn(xyz, k)[0] if idx is None else np.asarray(idx)
    r.C, r.finite = normals_ref.covariances(xyz, r.idx)
    w, v = np.linalg.eigh(r.C)
    r.evals = w
    n = v[:, :, 0].copy()
    n[np.trace(r.C, axis1=1, axis2=2) == 0] = (0.0, 0.0, 1.0)
    r.normal = n
    r.gap = normals_ref.gap_ratio(w)
    r.cov = regularised(n, epsilon)
    r.cov[~r.finite] = np.nan
    return r


def full(c6):
    """(m, 6) -> (m, 3, 3)"""
    c6 = np.asarray(c6, np.float64)
    M = np.empty((len(c6), 3, 3))
    for k, (a, b) in enumerate(_UPPER):
        M[:, a, b] = M[:, b, a] = c6[:, k]
    return M


# ------------------------------------------------------------------------------------------------------------ per pair
def mahalanobis(cs, ct, R):
    """(M (m, 6), ok (m,)) of m pairs: cs, ct (m, 6) float64, R (3, 3) float64 (the float32 rotation taken to double)."""
    cs, ct, R = np.asarray(cs, np.float64), np.asarray(ct, np.float64), np.asarray(R, np.float64)
    ok = np.isfinite(cs).all(axis=1) & np.isfinite(ct).all(axis=1)
    C = full(np.where(ok[:, None], cs, 0.0))
    T = np.where(ok[:, None], ct, 0.0)
    B = np.empty_like(C)
    for r in range(3):
        for c in range(3):
            B[:, r, c] = (R[r, 0] * C[:, 0, c] + R[r, 1] * C[:, 1, c]) + R[r, 2] * C[:, 2, c]
    A = np.empty((len(cs), 6))
    for k, (r, c) in enumerate(_UPPER):
        A[:, k] = T[:, k] + ((B[:, r, 0] * R[c, 0] + B[:, r, 1] * R[c, 1]) + B[:, r, 2] * R[c, 2])
    A00, A01, A02, A11, A12, A22 = A.T
    with np.errstate(all="ignore"):
        a00 = A11 * A22 - A12 * A12
        a01 = A02 * A12 - A01 * A22
        a02 = A01 * A12 - A02 * A11
        a11 = A00 * A22 - A02 * A02
        a12 = A01 * A02 - A00 * A12
        a22 = A00 * A11 - A01 * A01
        det = (A00 * a00 + A01 * a01) + A02 * a02
        inv = 1.0 / det
        M = np.stack([a00 * inv, a01 * inv, a02 * inv, a11 * inv, a12 * inv, a22 * inv], axis=1)
    ok = ok & np.isfinite(M).all(axis=1)
    M[~ok] = np.nan
    return M, ok


def pair_terms(p, q, M, ok, w, d2, X=None):
    """(m, 32) float64 terms of m pairs at the increment X: p, q float32 rows, M (m, 6) with ok, weights w, float32 d2."""
    X = np.eye(4) if X is None else np.asarray(X, np.float64)
    p = np.asarray(p, np.float32).astype(np.float64)
    q = np.asarray(q, np.float32).astype(np.float64)
    W = np.asarray(w, np.float64)
    Mm = full(np.where(np.asarray(ok)[:, None], M, 0.0))
    px, py, pz = p.T
    x = ((X[0, 0] * px + X[0, 1] * py) + X[0, 2] * pz) + X[0, 3]
    y = ((X[1, 0] * px + X[1, 1] * py) + X[1, 2] * pz) + X[1, 3]
    z = ((X[2, 0] * px + X[2, 1] * py) + X[2, 2] * pz) + X[2, 3]
    e = [q[:, 0] - x, q[:, 1] - y, q[:, 2] - z]
    g = [(Mm[:, r, 0] * e[0] + Mm[:, r, 1] * e[1]) + Mm[:, r, 2] * e[2] for r in range(3)]
    G = [[None] * 3 for _ in range(3)]
    for c in range(3):
        G[0][c] = y * Mm[:, 2, c] - z * Mm[:, 1, c]
        G[1][c] = z * Mm[:, 0, c] - x * Mm[:, 2, c]
        G[2][c] = x * Mm[:, 1, c] - y * Mm[:, 0, c]
    H = [[None] * 6 for _ in range(6)]
    for r in range(3):
        H[r][0] = G[r][2] * y - G[r][1] * z
        H[r][1] = G[r][0] * z - G[r][2] * x
        H[r][2] = G[r][1] * x - G[r][0] * y
        for c in range(3):
            H[r][3 + c] = G[r][c]
            H[3 + r][3 + c] = Mm[:, r, c]
    t = np.zeros((len(p), NUM_GICP_SUMS))
    t[:, 0] = W
    t[:, 1] = W * np.asarray(d2, np.float32).astype(np.float64)
    t[:, 2] = W
    t[:, 3] = W * ((e[0] * g[0] + e[1] * g[1]) + e[2] * g[2])
    k = 4
    for r in range(6):
        for c in range(r, 6):
            t[:, k] = W * H[r][c]
            k += 1
    t[:, 25] = W * (y * g[2] - z * g[1])
    t[:, 26] = W * (z * g[0] - x * g[2])
    t[:, 27] = W * (x * g[1] - y * g[0])
    t[:, 28] = W * g[0]
    t[:, 29] = W * g[1]
    t[:, 30] = W * g[2]
    t[~np.asarray(ok), 2:] = 0.0
    return t


def gicp_sums(p, q, M, ok, w, d2, X=None):
    """(sums, sum|term| per sum, terms per sum) over the given pairs at X."""
    t = pair_terms(p, q, M, ok, w, d2, X)
    cnt = np.full(NUM_GICP_SUMS, float(len(t)))
    cnt[2:] = float(np.asarray(ok).sum())
    return t.sum(axis=0), np.abs(t).sum(axis=0), cnt


def sums_bound(mag, cnt):
    """a sum of N terms, however ordered, is within (N + 16) * 2^-53 * sum|term| of the exact one (plane_ref.sums_bound)"""
    return (cnt + 16.0) * U * mag


# ------------------------------------------------------------------------------------------------------------ the inner loop
def delta(x):
    """PCL's constructTransformationMatrix in double: Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5), 4 x 4."""
    a, b, g = (float(v) for v in x[:3])
    sa, ca, sb, cb, sg, cg = math.sin(a), math.cos(a), math.sin(b), math.cos(b), math.sin(g), math.cos(g)
    D = np.eye(4)
    D[:3, :3] = [[cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca],
                 [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca],
                 [-sb, cb * sa, cb * ca]]
    D[:3, 3] = x[3:6]
    return D


def mul(A, B):
    """C = A B, entries ((a0 b0 + a1 b1) + a2 b2) + a3 b3, float64."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    C = np.empty((4, 4))
    for i in range(4):
        for j in range(4):
            C[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return C


def step(sums, scale=1.0):
    """(x, Delta(x), rank): x = scale * pinv(H) b over the eigen-directions above plane_ref.rank_cut."""
    _, rank, x = plane_ref.plane_solve(sums, want_x=True)
    if rank == 0:
        return np.zeros(6), np.eye(4), 0
    x = x * scale
    return x, delta(x), rank


def minimise(sums_at, prm, step_fn=step):
    """The step control of include/rsreg.h over any sums_at(X) -> 32 sums: (X, S, evaluations after the first)."""
    X = np.eye(4)
    S = np.asarray(sums_at(X), np.float64)
    evals = 0
    while int(S[0] + 0.5) >= 4 and evals < prm.max_inner_iterations:
        scale, accepted = 1.0, False
        x, D, rank = step_fn(S, scale)
        if rank == 0:
            break
        while evals < prm.max_inner_iterations:
            Xc = mul(D, X)
            Sc = np.asarray(sums_at(Xc), np.float64)
            evals += 1
            if Sc[3] <= S[3]:
                X, S, accepted = Xc, Sc, True
                break
            scale *= 0.5
            x, D, _ = step_fn(S, scale)
        if not accepted:
            break
        if (np.abs(x[:3]) <= prm.rotation_epsilon).all() and (np.abs(x[3:]) <= prm.transformation_epsilon).all():
            break
    return X, S, evals


def compose(X, T, prm):
    """(T_new float32, delta): T_new = float32(X T); PCL's test value over the 3 x 4 block."""
    T = np.asarray(T, np.float32)
    Tn = T.copy()
    Tn[:3] = mul(X, T.astype(np.float64))[:3].astype(np.float32)
    d = 0.0
    for r in range(3):
        for c in range(4):
            diff = abs(float(T[r, c]) - float(Tn[r, c]))
            eps = prm.rotation_epsilon if c < 3 else prm.transformation_epsilon
            with np.errstate(divide="ignore"):
                cd = 0.0 if diff == 0.0 else diff * float(np.float64(1.0) / np.float64(eps))
            if not (cd <= d):
                d = cd
    return Tn, d


class Gicp:
    """T (float32 4x4), converged, state, iterations, inner_evaluations, n_correspondences, mse, sums (of the last iteration),
    errors (|T - truth|_F per iteration when truth is given)"""


def gicp(src, tgt, cov_s, cov_t, guess=None, prm=None, truth=None, perturb=None, weights=None):
    prm = prm or Params()
    s = np.ascontiguousarray(src, np.float32)
    t = np.ascontiguousarray(tgt, np.float32)
    T = np.eye(4, dtype=np.float32) if guess is None else np.asarray(guess, np.float32).copy()
    fin = finite_rows(s)
    gate2 = float(prm.max_correspondence_distance) ** 2
    r = Gicp()
    r.iterations, r.inner_evaluations, r.state, r.converged, r.errors = 0, 0, "NOT_CONVERGED", False, []
    while True:
        cur = s.copy()
        if not (T == np.eye(4, dtype=np.float32)).all():
            cur[fin] = filters_ref.transform(s[fin], T)
        idx, d2 = plane_ref.nearest(cur, t, prm.max_correspondence_distance)
        k = np.flatnonzero((idx >= 0) & ~(d2.astype(np.float64) > gate2))
        M, ok = mahalanobis(cov_s[k], cov_t[idx[k]], T[:3, :3].astype(np.float64))
        W = np.ones(len(k)) if weights is None else np.asarray(weights, np.float64)[k]

        def sums_at(X):
            S = gicp_sums(cur[k], t[idx[k]], M, ok, W, d2[k], X)[0]
            if perturb is not None:
                S = S * (1.0 + perturb[1] * perturb[0].uniform(-1.0, 1.0, NUM_GICP_SUMS))
            return S
        X, S, evals = minimise(sums_at, prm)
        r.sums, r.n_correspondences = S, int(S[0] + 0.5)
        r.inner_evaluations += evals
        if r.n_correspondences < 4:
            r.state, r.converged = "NO_CORRESPONDENCES", False
            break
        r.mse = S[1] / S[0]
        T, d = compose(X, T, prm)
        r.iterations += 1
        if truth is not None:
            r.errors.append(float(np.linalg.norm(T.astype(np.float64) - truth)))
        if d < 1.0:
            r.state, r.converged = "TRANSFORM", True
            break
        if r.iterations >= prm.max_iterations:
            r.state, r.converged = "ITERATIONS", True
            break
    r.T = T
    return r
