"""A reference of GeneralizedIterativeClosestPoint6D as include/rsreg.h defines it (the GICP6D section), numpy only, independent
of the engine:

  * tables64 / lab: RGB -> normalised CIE L*a*b* from two GIVEN tables, every operation a float32 operation rounded once (numpy
    fuses nothing), in the header's order;
  * nearest6: the brute force in (x, y, z, c_L, c_a, c_b), c = w * lab' in float32 -- d6 = ((((dx^2 + dy^2) + dz^2) + dL^2) + da^2)
    + db^2 in float32, a NaN d6 skipped, ties to the lowest index, rejected iff double(d6) > gate^2; a query whose position or
    scaled colour is not finite gets no pair;
  * gicp6d: tests/gicp_ref.py's loop with that search in the place of the 3-D one; everything else is gicp_ref's own.
"""
import numpy as np

import filters_ref
import gicp_ref
from fitness_ref import finite_rows

F32 = np.float32
LAB_WEIGHT = 0.032   # PCL's default (recalled)


def tables64():
    """The two tables in float64: S (256), F (4000)."""
    f = np.arange(256) / 255.0
    S = np.where(f > 0.04045, ((f + 0.055) / 1.055) ** 2.4, f / 12.92)
    g = np.arange(4000) / 4000.0
    Ff = np.where(g > 0.008856, np.cbrt(g), 7.787 * g + 16.0 / 116.0)
    return S, Ff


def lab(S, Ftab, rgba):
    """(n, 3) float32 L / 100, a / 120, b / 120 of n packed rgb words, from the float32 tables S (256) and Ftab (4000)."""
    S, Ftab = np.asarray(S, F32), np.asarray(Ftab, F32)
    w = np.asarray(rgba, np.uint32).reshape(-1)
    r, g, b = S[(w >> 16) & 255], S[(w >> 8) & 255], S[w & 255]

    def mix(c0, c1, c2):
        return (r * F32(c0) + g * F32(c1)) + b * F32(c2)
    x, y, z = mix(0.412453, 0.357580, 0.180423), mix(0.212671, 0.715160, 0.072169), mix(0.019334, 0.119193, 0.950227)

    def f_of(v):
        return Ftab[np.clip((v * F32(4000.0)).astype(np.int32), 0, 3999)]
    fx, fy, fz = f_of(x / F32(0.95047)), f_of(y), f_of(z / F32(1.08883))
    L = np.minimum(F32(116.0) * fy - F32(16.0), F32(100.0))
    A = np.clip(F32(500.0) * (fx - fy), F32(-120.0), F32(120.0))
    B = np.clip(F32(200.0) * (fy - fz), F32(-120.0), F32(120.0))
    out = np.stack([L / F32(100.0), A / F32(120.0), B / F32(120.0)], axis=1)
    assert out.dtype == F32
    return out


def scaled(lab3, weight):
    """c = w * lab', w = float32(weight), one float32 multiply per coordinate"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (F32(weight) * np.ascontiguousarray(lab3, F32)[:, :3]).astype(F32)


def d6_f32(q, qc, t, tc):
    """float32 ((((dx^2 + dy^2) + dz^2) + dL^2) + da^2) + db^2 of broadcastable float32 arrays (last axis 3)"""
    d, c = q - t, qc - tc
    return ((((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + c[..., 0] * c[..., 0]) + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]


def nearest6(q, qc, t, tc, gate, chunk=256):
    """(index or -1 int32, float32 d6 or 0): the 6-D brute force over ALL finite target records.  q, t: (n, 3) float32 positions;
    qc, tc: the SCALED colours."""
    q, qc, t, tc = (np.ascontiguousarray(a, F32) for a in (q, qc, t, tc))
    idx = np.full(len(q), -1, np.int32)
    d2 = np.zeros(len(q), F32)
    tf = np.flatnonzero(finite_rows(t))
    rows = np.flatnonzero(finite_rows(q) & np.isfinite(qc).all(axis=1))
    if not len(tf) or not len(rows):
        return idx, d2
    gate2 = float(gate) * float(gate)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, len(rows), chunk):
            r = rows[s:s + chunk]
            d = d6_f32(q[r, None, :], qc[r, None, :], t[None, tf, :], tc[None, tf, :])
            d = np.where(np.isnan(d), np.inf, d).astype(F32)   # (a NaN d6 is skipped)
            a = d.argmin(axis=1)                               # (the first minimum: the lowest index)
            best = d[np.arange(len(r)), a]
            keep = np.isfinite(best) & ~(best.astype(np.float64) > gate2)
            idx[r[keep]] = tf[a[keep]]
            d2[r[keep]] = best[keep]
    return idx, d2


def gicp6d(src, tgt, lab_s, lab_t, cov_s, cov_t, weight=LAB_WEIGHT, guess=None, prm=None, truth=None, perturb=None):
    """gicp_ref.gicp with nearest6 as the correspondence search.  lab_s, lab_t: (n, 3) float32 L', a', b' per record."""
    prm = prm or gicp_ref.Params()
    s = np.ascontiguousarray(src, F32)
    t = np.ascontiguousarray(tgt, F32)
    cs6, ct6 = scaled(lab_s, weight), scaled(lab_t, weight)
    T = np.eye(4, dtype=F32) if guess is None else np.asarray(guess, F32).copy()
    fin = finite_rows(s)
    r = gicp_ref.Gicp()
    r.iterations, r.inner_evaluations, r.state, r.converged, r.errors = 0, 0, "NOT_CONVERGED", False, []
    while True:
        cur = s.copy()
        if not (T == np.eye(4, dtype=F32)).all():
            cur[fin] = filters_ref.transform(s[fin], T)
        idx, d2 = nearest6(cur, cs6, t, ct6, prm.max_correspondence_distance)
        k = np.flatnonzero(idx >= 0)
        M, ok = gicp_ref.mahalanobis(cov_s[k], cov_t[idx[k]], T[:3, :3].astype(np.float64))
        W = np.ones(len(k))

        def sums_at(X):
            S = gicp_ref.gicp_sums(cur[k], t[idx[k]], M, ok, W, d2[k], X)[0]
            if perturb is not None:
                S = S * (1.0 + perturb[1] * perturb[0].uniform(-1.0, 1.0, gicp_ref.NUM_GICP_SUMS))
            return S
        X, S, evals = gicp_ref.minimise(sums_at, prm)
        r.sums, r.n_correspondences = S, int(S[0] + 0.5)
        r.inner_evaluations += evals
        if r.n_correspondences < 4:
            r.state, r.converged = "NO_CORRESPONDENCES", False
            break
        r.mse = S[1] / S[0]
        T, d = gicp_ref.compose(X, T, prm)
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
