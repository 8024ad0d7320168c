"""CPU: the GICP reference (tests/gicp_ref.py, the numpy restatement of include/rsreg.h's rsreg_gicp_* contract) against
independent mathematics, the library's host-only entry points, and the whole-alignment cases the GPU test compares on.

  * C' = I - (1 - eps) n n^T against PCL's rule, U diag(1, 1, eps) U^T from numpy.linalg.svd, within 1e-12 on the records whose
    eigen-gap ratio is at least 1e-3 (the cut of tests/test_normals_gpu.py);
  * M against numpy.linalg.inv; a pair's 32 terms against J^T M J, J^T M e and e^T M e formed with matrices, and the cost's
    gradient by central differences: the header's formulas are the derivatives they claim to be;
  * rsreg_gicp_params_default, the struct sizes and rsreg_gicp_step_from_sums through the library (no GPU needed);
  * the alignment cases: the reference alone recovers the known motion, and it is robust to rounding -- with every evaluated sum
    perturbed by a relative 1e-12 the final transform moves by less than 1e-5 Frobenius, which is what lets the GPU comparison use
    the project's 1e-4 bar although the step control branches on a comparison of two sums.
"""
import ctypes as C

import numpy as np
import pytest

import gicp_cases as GC
import gicp_ref as G
import plane_ref
from plane_cases import source_near, three_walls

GAP_CUT = 1e-3   # tests/test_normals_gpu.py: where the normal's direction is asserted


def _uniform(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * np.array([2.0, 1.5, 0.7]) + np.array([-1.0, -0.5, 0.4])).astype(np.float32)


def _sphere(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return (np.array([0.1, -0.2, 1.5]) + (0.5 + 0.002 * rng.standard_normal(n))[:, None] * u).astype(np.float32)


@pytest.mark.parametrize("name,k", [("uniform", 20), ("sphere", 20), ("walls_noisy", 4), ("sphere", 64)])
def test_regularised_covariance_is_pcls_svd_rebuild(name, k):
    xyz = {"uniform": _uniform(1500, 1), "sphere": _sphere(1500, 3), "walls_noisy": source_near(three_walls(2000)[0], 1500)}[name]
    r = G.covariances(xyz, k, 1e-3)
    use = np.flatnonzero(r.finite & (r.gap >= GAP_CUT))
    assert len(use) >= 0.9 * len(xyz)
    want = np.stack([G.svd_rebuild(r.C[i], 1e-3) for i in use])
    err = np.abs(G.full(r.cov[use]) - want).max()
    print("%s k=%d: %d records, max |C' - U diag U^T| = %.3g" % (name, k, len(use), err))
    assert err <= 1e-12
    w = np.linalg.eigvalsh(G.full(r.cov[use]))
    assert np.abs(w - np.array([1e-3, 1.0, 1.0])).max() < 1e-12


def test_coincident_neighbours_and_non_finite_records():
    xyz = np.concatenate([np.repeat(np.array([[0.5, -0.25, 1.0]], np.float32), 30, axis=0), _uniform(100, 2)])
    xyz[40] = np.nan
    xyz[41, 1] = np.inf
    r = G.covariances(xyz, 20, 1e-3)
    flat = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1e-3])           # n = (0, 0, 1)
    assert np.abs(r.cov[:30] - flat).max() < 1e-15
    assert np.isnan(r.cov[40:42]).all() and np.isfinite(r.cov[42:]).all()


def _random_pairs(m, seed):
    rng = np.random.default_rng(seed)
    def unit(n):
        v = rng.standard_normal((n, 3))
        return v / np.linalg.norm(v, axis=1)[:, None]
    cs, ct = G.regularised(unit(m), 1e-3), G.regularised(unit(m), 1e-3)
    p = rng.uniform(-2, 2, (m, 3)).astype(np.float32)
    q = (p + rng.normal(0, 0.01, (m, 3))).astype(np.float32)
    R = plane_ref.euler_matrix(np.array([0.2, -0.1, 0.3, 0, 0, 0]))[:3, :3].astype(np.float64)
    return cs, ct, p, q, R, rng


def test_mahalanobis_is_the_inverse():
    cs, ct, _, _, R, _ = _random_pairs(200, 5)
    M, ok = G.mahalanobis(cs, ct, R)
    assert ok.all()
    want = np.linalg.inv(G.full(ct) + R @ G.full(cs) @ R.T)
    assert np.abs(G.full(M) - want).max() <= 1e-9 * np.abs(want).max()      # (cond of the sum is at most 1 / eps = 1e3)
    cs[3, 2] = np.nan
    ct[7, 0] = np.inf
    cs[9] = 0.0
    ct[9] = 0.0                                                             # singular: 1 / 0
    M, ok = G.mahalanobis(cs, ct, R)
    assert (~ok).nonzero()[0].tolist() == [3, 7, 9] and np.isnan(M[[3, 7, 9]]).all() and np.isfinite(M[ok]).all()


def test_pair_terms_are_the_normal_equations_of_the_objective():
    cs, ct, p, q, R, rng = _random_pairs(50, 6)
    M, ok = G.mahalanobis(cs, ct, R)
    w = rng.integers(1, 4, 50).astype(np.float64)
    d2 = plane_ref.d2_f32(p, q)
    X = GC.X_TEST
    t = G.pair_terms(p, q, M, ok, w, d2, X)
    Mf = G.full(M)
    for i in range(50):
        pp = X[:3, :3] @ p[i].astype(np.float64) + X[:3, 3]
        e = q[i].astype(np.float64) - pp
        skew = np.array([[0, -pp[2], pp[1]], [pp[2], 0, -pp[0]], [-pp[1], pp[0], 0]])
        J = np.hstack([-skew, np.eye(3)])
        H, b, c = J.T @ Mf[i] @ J, J.T @ Mf[i] @ e, e @ Mf[i] @ e
        A, bb = plane_ref.system(t[i])
        scale = max(1.0, np.abs(H).max())
        assert np.abs(A - w[i] * H).max() <= 1e-12 * w[i] * scale and np.abs(bb - w[i] * b).max() <= 1e-12 * w[i] * scale
        assert abs(t[i, 3] - w[i] * c) <= 1e-12 * w[i] * max(c, 1e-30) and t[i, 0] == t[i, 2] == w[i] and t[i, 31] == 0
        assert t[i, 1] == w[i] * float(d2[i])
    # the gradient of the cost along Delta(x) X at x = 0 is -2 b
    S = t.sum(axis=0)
    h = 1e-6
    for j in range(6):
        x = np.zeros(6)
        x[j] = h
        up = G.gicp_sums(p, q, M, ok, w, d2, G.mul(G.delta(x), X))[0][3]
        dn = G.gicp_sums(p, q, M, ok, w, d2, G.mul(G.delta(-x), X))[0][3]
        assert abs((up - dn) / (2 * h) + 2 * S[25 + j]) <= 1e-5 * max(1.0, abs(S[25 + j]))
    # a skipped pair adds to [0] and [1] only
    ok2 = ok.copy()
    ok2[::3] = False
    t2 = G.pair_terms(p, q, M, ok2, w, d2, X)
    assert (t2[::3, 2:] == 0).all() and (t2[::3, :2] == t[::3, :2]).all() and (t2[1::3] == t[1::3]).all()


def test_one_gauss_newton_step_lowers_the_cost():
    cs, ct, p, q, R, rng = _random_pairs(400, 7)
    T = plane_ref.euler_matrix(np.array([0.01, -0.02, 0.015, 0.01, -0.02, 0.005])).astype(np.float64)
    q = (p.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    M, ok = G.mahalanobis(cs, ct, R)
    w, d2 = np.ones(400), plane_ref.d2_f32(p, q)
    prm = G.Params(transformation_epsilon=1e-12, rotation_epsilon=1e-12, max_inner_iterations=20)
    X, S, evals = G.minimise(lambda X: G.gicp_sums(p, q, M, ok, w, d2, X)[0], prm)
    assert 2 <= evals <= 20 and S[3] < 1e-10 and np.abs(X - T).max() < 1e-6


# ---------------------------------------------------------------------------------------------------- through the library
@pytest.fixture(scope="module")
def L(rs):
    from rsreg_amd import lib
    lib.build()
    return lib


def test_params_default_and_struct_sizes(rs, L):
    from rsreg_amd import api
    assert C.sizeof(L.GicpParams) == 48
    assert C.sizeof(L.GicpResult) == 64 + 16 + 8 + 8 + 32 * 8 + 4 * 8 + 8
    p = api.gicp_params()
    assert (p.max_iterations, p.max_inner_iterations, p.k_correspondences) == (200, 20, 20)
    assert (p.max_correspondence_distance, p.transformation_epsilon, p.rotation_epsilon, p.gicp_epsilon) == (5.0, 5e-4, 2e-3, 1e-3)
    assert C.sizeof(L.IcpParams) == 64 and L.NUM_GICP_SUMS == 32


def test_host_step_matches_the_reference(rs, L):
    from rsreg_amd import api
    cs, ct, p, q, R, rng = _random_pairs(300, 8)
    M, ok = G.mahalanobis(cs, ct, R)
    S = G.gicp_sums(p, q, M, ok, np.ones(300), plane_ref.d2_f32(p, q))[0]
    for scale in (1.0, 0.25):
        x, D, rank = api.gicp_step_from_sums(S, scale)
        xr, Dr, rank_r = G.step(S, scale)
        assert rank == rank_r == 6
        assert np.abs(x - xr).max() <= 1e-10 * np.abs(xr).max() and np.abs(D - Dr).max() <= 1e-12
        assert (D[3] == (0, 0, 0, 1)).all()
    empty = np.zeros(32)
    x, D, rank = api.gicp_step_from_sums(empty)
    assert rank == 0 and not x.any() and (D == np.eye(4)).all()
    assert L.lib().rsreg_gicp_step_from_sums(None, 1.0, None, None, None) == L.RSREG_ERR_INVALID_ARG
    assert L.lib().rsreg_gicp_begin(None, None, None) == L.RSREG_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------------- whole alignments
@pytest.mark.parametrize("name", GC.ALIGN_CASES)
def test_reference_recovers_the_motion_and_is_robust_to_rounding(name):
    c = GC.align_case(name)
    ref = GC.align_reference(name)
    err = float(np.linalg.norm(ref.T.astype(np.float64) - c.truth))
    start = float(np.linalg.norm(np.eye(4) - c.truth))
    print("%s: %d iterations (%s), %d inner evaluations, %d pairs, |T - truth|_F %.3g (from %.3g), per iteration %s"
          % (name, ref.iterations, ref.state, ref.inner_evaluations, ref.n_correspondences, err, start, ["%.2g" % e for e in ref.errors]))
    assert ref.converged and ref.state == "TRANSFORM" and ref.iterations < c.prm.max_iterations
    assert ref.inner_evaluations <= ref.iterations * c.prm.max_inner_iterations
    assert err <= GC.TRUTH_MARGIN[name] and err < 0.05 * start
    moved = []
    for seed in (1, 2):
        got = G.gicp(c.src, c.tgt, c.cov_s, c.cov_t, None, c.prm, perturb=(np.random.default_rng(seed), 1e-12))
        moved.append(float(np.linalg.norm(got.T.astype(np.float64) - ref.T.astype(np.float64))))
    print("%s: sums perturbed by 1e-12 move the final transform by %s" % (name, ["%.3g" % m for m in moved]))
    assert max(moved) < 1e-5
