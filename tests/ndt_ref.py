"""A slow NDT written from the definition: the yardstick of tests/test_ndt_ref_cpu.py and tests/test_ndt_paths_gpu.py.

numpy float32 where a float32 step decides something discrete and has to be replayed bit for bit (the leaf of a point, the
radius test, PCL's running-sum centroid, the transform of the aligned cloud); exact integers and 60-digit mpmath for
everything that is mathematics.  It includes, calls and transcribes nothing of csrc/ndt_math.hpp, oracle/ndt_oracle.c or
the angle tables of PCL's computeAngleDerivatives: the derivatives of a transformed point come from differentiating the
three elementary rotations entry by entry (d/dt cos = -sin, d/dt sin = cos, constants to 0) and multiplying them out.

Grid.  leaf = floor_f32(x * inv_leaf) - float(min_b) per axis, key = i0 + i1 div0 + i2 div0 div1, the
voxels in ascending key order, those of fewer than 6 points dropped.  A voxel's moments are exact integers (every float32
is an integer multiple of 2^-149), so mean and

    cov = (n - 1) / n^2 * sum (x - m)(x - m)^T = (n - 1) (n sum x x^T - sum x sum x^T) / n^3

carry no cancellation error at all; eigen-decomposition (mpmath, 60 digits), the floor 0.01 * l_max on l_min (and then
on l_mid), the inverse through the eigenvectors.  A voxel whose exact l_max is 0 has no inverse: all zeros.

Score, gradient, Hessian (App. A.7).  Over the (point, voxel) incidence of the float32 radius test, fixed while
differentiating,

    score(p) = sum -d1 exp(-d2 / 2 * y^T S^-1 y),     y = R(p) x + t - mean,     R = Rx(p3) Ry(p4) Rz(p5)

The snap rule.  PCL evaluates the point Jacobian dR/dp x and the second derivatives d2R/dp dp x with cos = 1 and sin = 0
for an angle with |angle| < 10e-5 (pcl/registration/impl/ndt.hpp, computeAngleDerivatives, the three `if (std::abs(p(k))
< 10e-5)` tests at its head; SURVEY.md App. A.7 "small-angle snap"), while y is the point as transformPointCloud moved it,
at the true pose.  `derivatives()` therefore takes the derivative angles as an argument of their own, and `snap()` below is
that rule for its callers: strict <, on the absolute value, each angle for itself, 10e-5 being the double 1e-4.

Where PCL is not the derivative.  d2(R x)/d(ay)^2 has the first component -cy cz x - (-cy sz) y - sy z, i.e. the row
(-cy cz, cy sz, -sy); PCL's table row h_ang_d1 ends in +sy, and so do the engine (csrc/ndt_math.hpp) and the oracle, which
restate PCL.  The engine's contract is PCL's result, so `derivatives(pcl_d1=True)`, the default, adds 2 sin(ay) z to that
one component and says so; pcl_d1=False is the mathematics, and tests/test_ndt_ref_cpu.py shows that this single term is
all that separates the two (it vanishes under the snap, and it touches H[4][4] only).

Bounds (the derivations are in the docstring of `grid_bounds`).
"""
import math

import mpmath as mp
import numpy as np

mp.mp.dps = 60
f32 = np.float32
U = 2.0 ** -53

# ---- the measured tolerance of score / gradient / Hessian -----------------------------------------------------------------
# The kernel moves a point in float32 (pose angles and matrix rounded to float32, PCL's operation order); the ideal
# function moves it exactly.  DERIV_F32_GAP is the largest |sum(x' in f32) - sum(x' exact)| / sum|term| over the 28 sums
# (a term's magnitude over its addends: pair_sums) of every pass case of tests/ndt_cases.py, both sides this reference in 60 digits -- no kernel, no oracle took part.
# Measured 2026-10-17 by tests/test_ndt_ref_cpu.py::test_f32_gap_behind_the_bar (which measures it again and asserts that
# it has not outgrown the constant): 3.04e-6, set by the case `v1_n1_general` (one pair: nothing averages out).
# DERIV_BAR = 4 x that, for the order of the f64 summation and the f64 rounding of each term.
DERIV_F32_GAP = 3.1e-6
DERIV_BAR = 4.0 * DERIV_F32_GAP
# Against the reference at x' in FLOAT32 (the transform replayed bit for bit) and on the implementation's own table (its f64
# means and inverses, `with_table`; the table itself is judged by check_grid), nothing but f64 rounding is left, and the
# bound is derived, not measured: a term is a product of exp(-q) and a polynomial whose addends are reached by fewer than 64
# f64 operations; the inner products S y and S J_a round relative to |S| |y|, which exceeds |S y| by at most cond(S) <= 100
# (the floor: l_min >= 0.01 l_max); an error dq of the exponent is a relative error dq of exp(-q), and dq is q times the
# relative error of the quadratic form.  So a pair's term is off by at most 64 * 100 * u * (1 + q) of its magnitude, q its
# exponent; summed over the pairs that is F64_BAR * `fscale`, fscale = sum (1 + q) |term| from the reference (q is a few
# units where a term counts: about 1e-11 of the plain scale).
F64_OPS, F64_COND = 64, 100
F64_BAR = F64_OPS * F64_COND * U      # 7.1e-13, times fscale


SNAP = 10e-5
MIN_POINTS = 6
EIG_FLOOR = mp.mpf("0.01")


def snap(angles):
    """PCL's rule for the angles the derivatives are taken at: 0 (cos 1, sin 0) where |angle| < 10e-5."""
    return [0.0 if abs(float(a)) < SNAP else float(a) for a in angles]


def gauss_constants(res, outlier=0.55):
    res = mp.mpf(float(res))
    c1 = 10 * (1 - mp.mpf(outlier))
    c2 = mp.mpf(outlier) / res ** 3
    d3 = -mp.log(c2)
    d1 = -mp.log(c1 + c2) - d3
    d2 = -2 * mp.log((-mp.log(c1 * mp.exp(mp.mpf(-0.5)) + c2) - d3) / d1)
    return d1, d2


# ---- grid -----------------------------------------------------------------------------------------------------------------
def _exact_ints(a):
    """float32 array -> Python ints, each value times 2^149 (exact)."""
    return [int(v) for v in (np.asarray(a, np.float64) * 2.0 ** 149).ravel()]


def leaves(tgt, res):
    """(finite mask, key per finite point as int64, div as 3 Python ints, min_b): the float32 replay of the binning."""
    tgt = np.asarray(tgt, f32).reshape(-1, 3)
    fin = np.isfinite(tgt).all(1)
    t = tgt[fin]
    if len(t) == 0:
        return fin, np.zeros(0, np.int64), (0, 0, 0), (0, 0, 0)
    inv = f32(1.0) / f32(res)
    min_b = np.floor(t.min(0) * inv).astype(np.int64)
    div = np.floor(t.max(0) * inv).astype(np.int64) - min_b + 1
    ijk = (np.floor(t * inv) - min_b.astype(f32)).astype(np.int64)
    d0, d1, d2 = (int(v) for v in div)
    assert d0 * d1 * d2 < 2 ** 62
    key = ijk[:, 0] + ijk[:, 1] * d0 + ijk[:, 2] * (d0 * d1)
    return fin, key, (d0, d1, d2), tuple(int(v) for v in min_b)


def _inv_from_eig(lam, Q):
    out = mp.matrix(3, 3)
    for r in range(3):
        for c in range(3):
            out[r, c] = sum(Q[r, k] * Q[c, k] / lam[k] for k in range(3))
    return out


def grid(tgt, res):
    """The voxel grid of a target.  Returns a dict: div, n_leaves, occupied (leaves holding a finite point), counts of
    the occupied leaves in key order, and per KEPT voxel (count >= 6) in key order: n, mean / cov / icov (mpmath, cov the
    floored one where the floor applied), lam (exact l_min, l_mid, l_max before the floor), floored, sxx (sum x_k^2 per
    axis, f64), sabs (sum |x_k|), cen_mean (the exact mean rounded to float32) and cen_pcl (PCL's sequential float sum in
    input order / float(n))."""
    tgt = np.asarray(tgt, f32).reshape(-1, 3)
    fin, key, div, min_b = leaves(tgt, res)
    t = tgt[fin]
    order = np.argsort(key, kind="stable")
    ks, start = np.unique(key[order], return_index=True)
    bounds = list(start) + [len(order)]
    g = {"div": div, "n_leaves": div[0] * div[1] * div[2], "occupied": len(ks), "n_finite": int(fin.sum()),
         "occupied_counts": np.diff(bounds).astype(np.int64), "vox": []}
    scale = mp.mpf(2) ** 149
    for j in range(len(ks)):
        pts = t[order[bounds[j]:bounds[j + 1]]]          # input order: the sort is stable
        n = len(pts)
        if n < MIN_POINTS:
            continue
        X = [_exact_ints(pts[:, k]) for k in range(3)]
        S = [sum(x) for x in X]
        mean = mp.matrix([mp.mpf(S[k]) / (n * scale) for k in range(3)])
        cov = mp.matrix(3, 3)
        for r in range(3):
            for c in range(r, 3):
                sxy = sum(a * b for a, b in zip(X[r], X[c]))
                cov[r, c] = cov[c, r] = mp.mpf((n - 1) * (n * sxy - S[r] * S[c])) / (mp.mpf(n) ** 3 * scale * scale)
        E, Q = mp.eigsy(cov)
        lam = sorted(((E[i], i) for i in range(3)), key=lambda e: e[0])
        Q = mp.matrix([[Q[r, lam[k][1]] for k in range(3)] for r in range(3)])
        lam = [max(l[0], mp.mpf(0)) for l in lam]        # (a PSD matrix: anything below 0 is the solver's last digit)
        exact = list(lam)
        floored = False
        icov = mp.matrix(3, 3)
        if lam[2] > 0:
            fl = EIG_FLOOR * lam[2]
            if lam[0] < fl:
                floored = True
                lam[0] = fl
                if lam[1] < fl:
                    lam[1] = fl
                for r in range(3):
                    for c in range(3):
                        cov[r, c] = sum(Q[r, k] * lam[k] * Q[c, k] for k in range(3))
            icov = _inv_from_eig(lam, Q)
        s = f32(0), f32(0), f32(0)
        for p in pts:
            s = s[0] + p[0], s[1] + p[1], s[2] + p[2]
        d = pts.astype(np.float64)
        g["vox"].append({"n": n, "mean": mean, "cov": cov, "icov": icov, "lam": exact, "lam_floored": lam, "floored": floored,
                         "sxx": (d * d).sum(0), "sabs": np.abs(d).sum(0),
                         "cen_mean": np.array([f32(float(mean[k])) for k in range(3)], f32),
                         "cen_pcl": np.array([s[k] / f32(n) for k in range(3)], f32)})
    return g


def as_table(g):
    """(m (V x 21 f64: mean, cov, icov), counts) in the layout of voxels()."""
    V = len(g["vox"])
    m = np.zeros((V, 21))
    for j, v in enumerate(g["vox"]):
        m[j, 0:3] = [float(v["mean"][k]) for k in range(3)]
        m[j, 3:12] = [float(v["cov"][r, c]) for r in range(3) for c in range(3)]
        m[j, 12:21] = [float(v["icov"][r, c]) for r in range(3) for c in range(3)]
    return m, np.array([v["n"] for v in g["vox"]], np.int32)


def with_table(g, m):
    """The grid `g` with every voxel's mean and inverse covariance replaced by the f64 values of an implementation's table
    `m` (the layout of voxels()), exactly: what a pass that reads that table is to be judged on."""
    assert len(m) == len(g["vox"])
    out = dict(g)
    out["vox"] = []
    for j, v in enumerate(g["vox"]):
        w = dict(v)
        w["mean"] = mp.matrix([mp.mpf(float(x)) for x in m[j, 0:3]])
        w["icov"] = mp.matrix([[mp.mpf(float(m[j, 12 + 3 * r + c])) for c in range(3)] for r in range(3)])
        out["vox"].append(w)
    return out


def grid_bounds(v):
    """Bounds on what an f64 single pass may make of voxel `v`, from the exact moments alone.

    With u = 2^-53 and g = gamma_n = n u / (1 - n u), any order of adding n f64 terms gives fl(sum) = sum + e,
    |e| <= g sum|term|.  Mean: m_k = fl(S_k / n), so |dm_k| <= (g + u) sum|x_k| / n.

    Covariance, PCL's single pass ((Sxy - 2 S_r m_c) / n + m_r m_c) (n - 1) / n.  Let Q = sqrt(sum x_r^2 sum x_c^2); by
    Cauchy-Schwarz sum|x_r x_c| <= Q, |S_r m_c| <= Q and |m_r m_c| <= Q / n.  Then: Sxy carries g Q; S_r m_c has a relative
    error 2 g + 2 u, doubled exactly: (4 g + 4 u) Q; the subtraction rounds at u (|Sxy| + 2 |S_r m_c|) <= 3 u Q; the
    division by n adds u 3 Q / n; m_r m_c carries (2 g + 3 u) Q / n, the addition u 4 Q / n, the factor (n - 1) / n two
    more roundings of the whole.  Summed over n and rounded up:  |dcov_rc| <= (5 g + 16 u) Q / n.

    Inverse.  Relative error of the (floored) covariance times its condition number times the size of the inverse:
    |dC| l_max / l_min * 1 / l_max * 1 / l_min = |dC| / l_min^2 (first order in dC), with |dC| the Frobenius norm of the
    bound above -- times 1 + 2 (floor - l_min) / gap where the floor applied, since the rebuilt matrix then also moves
    with the eigenvector of l_min, which a perturbation dC turns by |dC| / gap (gap: to the nearest eigenvalue NOT
    floored with it) -- plus the f64 rounding of the eigen-decomposition, the rebuild and the adjugate inverse, whose
    cofactors cancel at u l_max^2 against a determinant l_min l_mid l_max: 64 u l_max / (l_min l_mid).
    Returns (mean bound [3], cov bound [3 x 3], icov bound scalar, lam_min_is_above_cov_bound)."""
    n = v["n"]
    g = n * U / (1 - n * U)
    mean_b = (g + U) * v["sabs"] / n
    Q = np.sqrt(np.outer(v["sxx"], v["sxx"]))
    cov_b = (5 * g + 16 * U) * Q / n
    dC = float(np.linalg.norm(cov_b))
    l0, l1, l2 = (float(x) for x in v["lam_floored"])
    e0, e1, e2 = (float(x) for x in v["lam"])
    well = e0 > dC
    if l2 <= 0:
        return mean_b, cov_b, 0.0, well
    amp = 1.0
    if v["floored"]:
        gap = (e1 - e0) if e1 >= 0.01 * e2 else (e2 - e1)
        amp += 2 * (l0 - e0) / gap if gap > 0 else math.inf
    icov_b = dC * amp / (l0 * l0) + 64 * U * l2 / (l0 * l1)
    return mean_b, cov_b, icov_b, well


def check_grid(c, g, m, cnt, cen, pcl_mode, oracle_m=None):
    """voxels() / centroids() of an implementation against the reference grid `g` within ndt_ref.grid_bounds."""
    rm, rc = as_table(g)
    np.testing.assert_array_equal(cnt, rc)
    assert m.shape == rm.shape
    want = np.array([v["cen_pcl" if pcl_mode else "cen_mean"] for v in g["vox"]], np.float32).reshape(-1, 3)
    np.testing.assert_array_equal(np.asarray(cen, np.float32).view(np.uint32), want.view(np.uint32))
    for j, v in enumerate(g["vox"]):
        mean_b, cov_b, icov_b, well = grid_bounds(v)
        assert well or c["degenerate"], (c["name"], j, "a well-posed case must not leave the floor to a rounding error")
        assert (np.abs(m[j, 0:3] - rm[j, 0:3]) <= mean_b).all(), (c["name"], j, "mean")
        ic, ric = m[j, 12:21], rm[j, 12:21]
        if well:
            l0, l2 = float(v["lam_floored"][0]), float(v["lam_floored"][2])
            amp = icov_b * l0 * l0 if v["floored"] else 0.0          # (the floored covariance moves with the eigenvectors too)
            assert (np.abs(m[j, 3:12] - rm[j, 3:12]).reshape(3, 3) <= cov_b + amp + 16 * U * l2).all(), (c["name"], j, "cov")
            assert np.abs(ic - ric).max() <= icov_b, (c["name"], j, "icov", np.abs(ic - ric).max(), icov_b)
        else:
            # l_min is 0 up to rounding: PCL's `ev < 0` may go either way; kept -> the floored inverse, dropped -> zeros
            if oracle_m is not None:
                assert bool(ic.any()) == bool(oracle_m[j, 12:21].any()), (c["name"], j, "the choice differs from the oracle's")
            if ic.any():
                assert float(v["lam"][2]) > 0 and np.abs(ic - ric).max() <= icov_b, (c["name"], j, np.abs(ic - ric).max(), icov_b)
            else:
                assert not ic.any()


# ---- transform ------------------------------------------------------------------------------------------------------------
def _mul4(a, b):
    r = np.zeros((4, 4), f32)
    for i in range(4):
        for j in range(4):
            s = a[i, 0] * b[0, j]
            for k in (1, 2, 3):
                s = f32(s + a[i, k] * b[k, j])
            r[i, j] = s
    return r


def pose_matrix_f32(p):
    """Translation * Rx * Ry * Rz as PCL assembles it in float32: angles rounded to float32, their sine and cosine rounded
    to float32, the products left to right, each entry a left-to-right float32 sum of four products."""
    cs = []
    for k in (3, 4, 5):
        a = mp.mpf(float(f32(p[k])))
        cs.append((f32(float(mp.cos(a))), f32(float(mp.sin(a)))))
    (cx, sx), (cy, sy), (cz, sz) = cs
    one = lambda: np.eye(4, dtype=f32)
    Rx, Ry, Rz, Tr = one(), one(), one(), one()
    Rx[1, 1], Rx[1, 2], Rx[2, 1], Rx[2, 2] = cx, -sx, sx, cx
    Ry[0, 0], Ry[0, 2], Ry[2, 0], Ry[2, 2] = cy, sy, -sy, cy
    Rz[0, 0], Rz[0, 1], Rz[1, 0], Rz[1, 1] = cz, -sz, sz, cz
    Tr[:3, 3] = [f32(p[0]), f32(p[1]), f32(p[2])]
    return _mul4(_mul4(_mul4(Tr, Rx), Ry), Rz)


def transform_f32(M, xyz):
    """((M0 x + M1 y) + M2 z) + M3 per row, every step rounded to float32: the operation order of the pass and of
    the aligned cloud."""
    M = np.asarray(M, f32)
    x, y, z = (np.asarray(xyz, f32)[:, k] for k in range(3))
    with np.errstate(all="ignore"):
        return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], axis=1).astype(f32)


def incidence(xf, cen, res):
    """[n x V] bool: the float32 radius test (dx^2 + dy^2) + dz^2 < float(res^2) of moved points against centroids, and
    the smallest |dd - r2| / r2 (how far the nearest pair is from changing sides)."""
    r2 = f32(float(res) * float(res))
    xf, cen = np.asarray(xf, f32), np.asarray(cen, f32).reshape(-1, 3)
    d = xf[:, None, :] - cen[None, :, :]
    dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    margin = float(np.min(np.abs(dd - r2)) / r2) if dd.size else math.inf
    return dd < r2, margin


def _elem(axis, t, order):
    """The `order`-th derivative of the elementary rotation about `axis` by t: cos and sin entries differentiated
    (d^k/dt^k cos t = cos(t + k pi / 2)), the constant entries 1 and 0 differentiated to 0."""
    t = mp.mpf(t)
    if t == 0:   # (the snapped angle: cos 1, sin 0 exactly, whatever pi is rounded to)
        c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][order % 4]
        c, s = mp.mpf(c), mp.mpf(s)
    else:
        c, s = mp.cos(t + order * mp.pi / 2), mp.sin(t + order * mp.pi / 2)
    k = mp.mpf(1 if order == 0 else 0)
    if axis == 0:
        return mp.matrix([[k, 0, 0], [0, c, -s], [0, s, c]])
    if axis == 1:
        return mp.matrix([[c, 0, s], [0, k, 0], [-s, 0, c]])
    return mp.matrix([[c, -s, 0], [s, c, 0], [0, 0, k]])


def rotation(angles, orders=(0, 0, 0)):
    """d^(o0 + o1 + o2) / dax^o0 day^o1 daz^o2 of Rx(ax) Ry(ay) Rz(az)."""
    return _elem(0, angles[0], orders[0]) * _elem(1, angles[1], orders[1]) * _elem(2, angles[2], orders[2])


_PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]
_TERMS = {}    # point_terms by its arguments: a case is evaluated on more than one table, its points are moved once


def point_terms(src, pose, dangles, xprime="exact", pcl_d1=True):
    """Per point: y0 = the moved point (mpmath 3-vector; `f32`: PCL's float32 transform replayed, `exact`: R(p) x + t in
    60 digits), J (6 vectors: dx'/dp_a at the derivative angles) and H (dict (a, b) -> vector, a <= b, both >= 3).
    pcl_d1: the one place where PCL is not the derivative (see the module docstring)."""
    src = np.asarray(src, f32).reshape(-1, 3)
    key = (src.tobytes(), tuple(float(a) for a in pose), tuple(float(a) for a in dangles), xprime, pcl_d1)
    if key in _TERMS:
        return _TERMS[key]
    dR = [rotation(dangles, o) for o in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
    ddR = {(3, 3): rotation(dangles, (2, 0, 0)), (3, 4): rotation(dangles, (1, 1, 0)), (3, 5): rotation(dangles, (1, 0, 1)),
           (4, 4): rotation(dangles, (0, 2, 0)), (4, 5): rotation(dangles, (0, 1, 1)), (5, 5): rotation(dangles, (0, 0, 2))}
    if xprime == "f32":
        moved = transform_f32(pose_matrix_f32(pose), src).astype(np.float64)
    else:
        R = rotation([float(a) for a in pose[3:6]])
        t = mp.matrix([mp.mpf(float(a)) for a in pose[0:3]])
    unit = [mp.matrix([1, 0, 0]), mp.matrix([0, 1, 0]), mp.matrix([0, 0, 1])]
    out = []
    for i in range(len(src)):
        x = mp.matrix([mp.mpf(float(v)) for v in src[i]])
        y0 = mp.matrix([mp.mpf(float(v)) for v in moved[i]]) if xprime == "f32" else R * x + t
        H = {k: d * x for k, d in ddR.items()}
        if pcl_d1:
            H[(4, 4)][0] += 2 * mp.sin(mp.mpf(dangles[1])) * x[2]   # -sin(ay) x_z, the derivative, becomes PCL's +sin(ay) x_z
        out.append((y0, unit + [d * x for d in dR], H))
    if len(_TERMS) >= 64:
        _TERMS.clear()
    _TERMS[key] = out
    return out


def pair_sums(y0, J, H, vox, d1, d2):
    """The 28 terms of one (point, voxel) pair: score, gradient (6), upper triangle of the Hessian (21) -- the chain rule
    on -d1 exp(-d2 / 2 y^T S^-1 y) with dy/dp_a = J_a and d2y/dp_a dp_b = H_ab; None where PCL skips the pair
    (d2 e outside [0, 1]).  With them the magnitude of each term, taken over its addends (|c_r J_ar| of the gradient's dot
    product; the three addends of a Hessian entry): the scale errors are measured against, which a pair whose addends
    happen to cancel must not shrink -- a sum of one pair would otherwise have no scale at all.  Third: the exponent q."""
    S = vox["icov"]
    y = y0 - vox["mean"]
    c = S * y
    expo = d2 * (y.T * c)[0] / 2
    e = mp.exp(-expo)
    if d2 * e > 1 or d2 * e < 0:
        return None
    k = d1 * d2 * e
    cj = [(c.T * J[a])[0] for a in range(6)]
    SJ = [S * J[a] for a in range(6)]
    out = [-d1 * e] + [k * cj[a] for a in range(6)]
    mag = [abs(d1 * e)] + [abs(k) * sum(abs(c[r] * J[a][r]) for r in range(3)) for a in range(6)]
    for a, b in _PAIRS:
        h = (c.T * H[(a, b)])[0] if a >= 3 else mp.mpf(0)
        q, jsj = -d2 * cj[a] * cj[b], (J[b].T * SJ[a])[0]
        out.append(k * (q + h + jsj))
        mag.append(abs(k) * (abs(q) + abs(h) + abs(jsj)))
    return out, mag, expo


def derivatives(src, g, res, pose, dangles=None, xprime="exact", centroids="cen_mean", pcl_d1=True):
    """Score, gradient and Hessian of NDT over grid `g` (of `grid()`), as per-point rows so that any multiset of the points
    can be summed by its caller.  dangles: the angles the point derivatives are taken at (default: snap(pose[3:6])).
    Returns a dict: rows ([n][28] mpmath, None for a point without a pair), abs ([n][28] sum |term|), inc (the incidence),
    margin (of the radius test), sums / scale / fscale (28 f64 each: the totals, of the terms, of their magnitudes, of
    (1 + q) times their magnitudes), pairs."""
    src = np.asarray(src, f32).reshape(-1, 3)
    dangles = snap(pose[3:6]) if dangles is None else dangles
    fin = np.isfinite(src).all(1)
    safe = np.where(fin[:, None], src, f32(0))
    cen = np.array([v[centroids] for v in g["vox"]], f32).reshape(-1, 3)
    inc, margin = incidence(transform_f32(pose_matrix_f32(pose), safe), cen, res)
    inc &= fin[:, None]
    d1, d2 = gauss_constants(res)
    rows, absr, absq, pairs = [], [], [], 0
    need = np.flatnonzero(inc.any(1))
    terms = dict(zip(need, point_terms(safe[need], pose, dangles, xprime, pcl_d1)))
    for i in range(len(src)):
        if i not in terms:
            rows.append(None)
            absr.append(None)
            absq.append(None)
            continue
        y0, J, H = terms[i]
        acc, aab, aaq = [mp.mpf(0)] * 28, [mp.mpf(0)] * 28, [mp.mpf(0)] * 28
        for j in np.flatnonzero(inc[i]):
            t = pair_sums(y0, J, H, g["vox"][j], d1, d2)
            if t is None:
                continue
            pairs += 1
            acc = [a + b for a, b in zip(acc, t[0])]
            aab = [a + b for a, b in zip(aab, t[1])]
            aaq = [a + (1 + t[2]) * b for a, b in zip(aaq, t[1])]
        rows.append(acc)
        absr.append(aab)
        absq.append(aaq)
    out = {"rows": rows, "abs": absr, "absq": absq, "inc": inc, "margin": margin, "pairs": pairs}
    out["sums"], out["scale"], out["fscale"] = total(out, np.ones(len(src), np.int64))
    return out


def total(d, mult):
    """sum_i mult[i] * row_i, the same of the absolute terms and of (1 + q) times them, as 28 f64 each."""
    acc = [[mp.mpf(0)] * 28 for _ in range(3)]
    for i, m in enumerate(mult):
        if m and d["rows"][i] is not None:
            for k, key in enumerate(("rows", "abs", "absq")):
                acc[k] = [a + int(m) * b for a, b in zip(acc[k], d[key][i])]
    return tuple(np.array([float(a) for a in r]) for r in acc)


def unpack(s):
    """28 sums -> (score, gradient [6], Hessian [6 x 6])."""
    h = np.zeros((6, 6))
    for k, (a, b) in enumerate(_PAIRS):
        h[a, b] = h[b, a] = s[7 + k]
    return float(s[0]), np.asarray(s[1:7], np.float64), h


def pack(score, grad, hess):
    hess = np.asarray(hess, np.float64).reshape(6, 6)
    return np.array([score] + list(np.asarray(grad, np.float64)) + [hess[a, b] for a, b in _PAIRS])
