"""A slow Umeyama (rigid, no scaling) written from the definition in 60-digit arithmetic (mpmath): the yardstick of
tests/test_umeyama_cpu.py and tests/test_umeyama_gpu.py.  It shares no code and no construction with csrc/host_linalg.hpp or
oracle/orc_linalg.h: the SVD is mpmath's (Golub-Kahan), nothing is completed by hand, and rank is the caller's business.

    sigma = 1/n sum (q_i - mu_q)(p_i - mu_p)^T = U diag(s) V^T,   R = U diag(1, 1, sign(det U det V)) V^T,   t = mu_q - R mu_p

Also the two neighbours NDT runs on the host: a symmetric 3 x 3 eigen-decomposition and the 6 x 6 pseudo-inverse solve with
Eigen's rank rule (s_i > 6 eps s_max).

The bound of a well-posed case (test_umeyama_cpu.py states where each term comes from):

    |R - R_ref| <= ulp32(R_ref) / 2 + e,    |t - t_ref| <= ulp32(t_ref) / 2 + e (1 + |mu_p|),
    e = C 2^-52 (kappa + (family `far` only) |mu_q| |mu_p| / s2),   kappa = s1 / (s2 + s3), or s1 / (s2 - s3) where det U det V < 0
"""
import mpmath as mp
import numpy as np

mp.mp.dps = 60

# The one constant of the bound, for all families: 4 x the larger of two measured ratios, worst entry of error / bound-with-C=1
# (tests/test_umeyama_cpu.py::test_measured_ratios_behind_C measures both again and asserts that neither has outgrown C / 4):
#   RATIO_SUMS_VS_PAIRS  reference from the 17 sums against reference from the pairs, both mpmath, every well-posed row of the
#                        table: what adding n terms in f64 costs before any solver has run (the worst rows are `far` at
#                        n = 1000, where it is the cancellation term itself that the summation outgrows: C scales that term too)
#   RATIO_HOST_FULL      cold host form against the reference from the pairs, family `full`
RATIO_SUMS_VS_PAIRS = 1.470
RATIO_HOST_FULL = 0.973
C = 4.0 * max(RATIO_SUMS_VS_PAIRS, RATIO_HOST_FULL)

EPS = 2.0 ** -52


def _m(a):
    a = np.asarray(a)
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in a.reshape(a.shape[0], -1)])


def _np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)], np.float64)


def _solve(sigma, mu_p, mu_q):
    U, S, Vt = mp.svd_r(sigma, compute_uv=True)   # sigma = U diag(S) Vt, S descending
    one = mp.eye(3)
    assert mp.mnorm(U.T * U - one, "inf") < mp.mpf(10) ** -45 and mp.mnorm(Vt * Vt.T - one, "inf") < mp.mpf(10) ** -45
    sign = 1 if mp.det(U) * mp.det(Vt) > 0 else -1
    R = U * mp.diag([1, 1, sign]) * Vt
    t = mu_q - R * mu_p
    return {"R": _np(R), "t": _np(t).ravel(), "s": np.array([float(S[i]) for i in range(3)]), "sign": sign,
            "mu_p": _np(mu_p).ravel(), "mu_q": _np(mu_q).ravel(), "_R": R, "_t": t}


def from_pairs(P, Q):
    """P -> Q (n x 3 each, any float type, taken exactly): centre first, then the covariance."""
    P, Q = _m(P), _m(Q)
    n = P.rows
    mu_p = mp.matrix(3, 1)
    mu_q = mp.matrix(3, 1)
    for i in range(n):
        for k in range(3):
            mu_p[k] += P[i, k]
            mu_q[k] += Q[i, k]
    mu_p /= n
    mu_q /= n
    sigma = mp.matrix(3, 3)
    for i in range(n):
        for r in range(3):
            dq = Q[i, r] - mu_q[r]
            for c in range(3):
                sigma[r, c] += dq * (P[i, c] - mu_p[c])
    sigma /= n
    return _solve(sigma, mu_p, mu_q)


def from_sums(sums):
    """The same from the 17 sums (n, sum p, sum q, sum q_i p_j row-major, sum d^2), each an exact f64."""
    s = [mp.mpf(float(x)) for x in sums]
    n = s[0]
    mu_p = mp.matrix([s[1 + k] / n for k in range(3)])
    mu_q = mp.matrix([s[4 + k] / n for k in range(3)])
    sigma = mp.matrix(3, 3)
    for r in range(3):
        for c in range(3):
            sigma[r, c] = s[7 + 3 * r + c] / n - mu_q[r] * mu_p[c]
    return _solve(sigma, mu_p, mu_q)


def rms_residual(P, Q, R, t):
    """sqrt(1/n sum |q_i - (R p_i + t)|^2), R and t taken exactly."""
    P, Q, R = _m(P), _m(Q), _m(R)
    t = mp.matrix([mp.mpf(float(x)) for x in np.asarray(t).ravel()])
    acc = mp.mpf(0)
    for i in range(P.rows):
        for r in range(3):
            d = Q[i, r] - (R[r, 0] * P[i, 0] + R[r, 1] * P[i, 1] + R[r, 2] * P[i, 2] + t[r])
            acc += d * d
    return float(mp.sqrt(acc / P.rows))


def ulp32(x):
    """The spacing of float32 at |x|, elementwise, as f64."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def kappa(ref):
    """The conditioning of the polar factor: s1 / (s2 + s3), s1 / (s2 - s3) where det U det V < 0 (inf where that is 0)."""
    s = ref["s"]
    d = s[1] + ref["sign"] * s[2]
    return float(s[0] / d) if d > 0 else float("inf")


def bound(ref, far=False, c=None):
    """Per-entry bound on |T - T_ref| of a well-posed case, as a 4 x 4 array (row 3: zero, that row is exact)."""
    c = C if c is None else c
    k = kappa(ref)
    nmp, nmq = float(np.linalg.norm(ref["mu_p"])), float(np.linalg.norm(ref["mu_q"]))
    r_err = c * EPS * (k + (nmq * nmp / ref["s"][1] if far else 0.0))
    B = np.zeros((4, 4))
    B[:3, :3] = 0.5 * ulp32(ref["R"]) + r_err
    B[:3, 3] = 0.5 * ulp32(ref["t"]) + r_err * (1.0 + nmp)
    return B


def T_of(ref):
    T = np.eye(4)
    T[:3, :3] = ref["R"]
    T[:3, 3] = ref["t"]
    return T


def eig_sym3(A):
    """Eigenvalues ascending and eigenvectors in columns of a symmetric 3 x 3."""
    E, Q = mp.eigsy(_m(np.asarray(A, np.float64).reshape(3, 3)))
    return np.array([float(E[i]) for i in range(3)]), _np(Q)


def pinv_solve6(A, b):
    """x = pinv(A) b, 6 x 6, singular values kept where s_i > 6 eps s_max.  Returns x, s, the coefficients (u_k . b) / s_k of
    x along the right singular vectors (0 where s_k is 0) and those vectors in columns."""
    U, S, Vt = mp.svd_r(_m(np.asarray(A, np.float64).reshape(6, 6)), compute_uv=True)
    bb = mp.matrix([mp.mpf(float(x)) for x in b])
    s = [S[i] for i in range(6)]
    thr = 6 * mp.mpf(2) ** -52 * s[0]
    x = mp.matrix(6, 1)
    coef = []
    for k in range(6):
        d = sum(U[i, k] * bb[i] for i in range(6)) / s[k] if s[k] > 0 else mp.mpf(0)
        coef.append(float(d))
        if s[k] > thr and s[k] > 0:
            for i in range(6):
                x[i] += Vt[k, i] * d
    return _np(x).ravel(), np.array([float(v) for v in s]), np.array(coef), _np(Vt.T)
