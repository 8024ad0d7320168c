"""CPU: the arithmetic of point-to-plane ICP (include/rsreg.h: RSREG_NUM_PLANE_SUMS) without a GPU -- the numpy reference
against exact rational arithmetic, the library's host-only solve (rsreg_plane_solve_from_sums) against numpy.linalg.lstsq on
full-rank and degenerate systems and on both sides of its rank cut, the condition the GPU alignment test relies on (on the
50 k synthetic "bench" pair point-to-plane is no further from the ground truth than point-to-point after 10 iterations),
and the ABI."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import plane_ref

F32_EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def L(rs):
    from rsreg_amd import lib
    lib.build()
    return lib


def walls(rng, planes, per_plane=200, noise=0.0):
    """Target points on axis-aligned planes [(axis, value)], their normals, and the (n, 3) float32 arrays."""
    q, n = [], []
    for axis, value in planes:
        p = rng.uniform(-1.0, 1.0, (per_plane, 3))
        p[:, 2] += 1.5
        p[:, axis] = value
        nn = np.zeros((per_plane, 3))
        nn[:, axis] = 1.0
        q.append(p)
        n.append(nn)
    return np.concatenate(q).astype(np.float32), np.concatenate(n).astype(np.float32)


def moved_source(q, x, rng, slide=0.01):
    """Source points: the target points slid along nothing in particular, moved by the INVERSE of the small motion x."""
    T = plane_ref.euler_matrix(x).astype(np.float64)
    Ti = np.linalg.inv(T)
    p = q.astype(np.float64) + rng.uniform(-slide, slide, q.shape)
    return (p @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)


def lstsq_solution(p, q, n):
    """x of min |J x - r| over the pairs (minimum norm where the system is singular), float64."""
    t, _ = plane_ref.pair_terms(p, q, n, np.ones(len(p)), np.zeros(len(p), np.float32))
    p64, q64, n64 = (a.astype(np.float64) for a in (p, q, n))
    J = np.concatenate([np.cross(p64, n64), n64], axis=1)
    r = np.einsum("ij,ij->i", n64, q64 - p64)
    x = np.linalg.lstsq(J, r, rcond=None)[0]
    return x, J


def solve_tolerance(T, cond):
    """entries within cond * 2^-50 (the solve's conditioning) plus one float rounding of the entry"""
    return cond * 2.0 ** -50 + F32_EPS * np.maximum(np.abs(T), 1.0)


def test_plane_sums_match_exact_rational_arithmetic():
    """Against fractions.Fraction on 200 random pairs, in the two steps the arithmetic has.  The ADDITIONS: every sum is within
    (n + 16) * 2^-53 * sum|term| of the exact sum of its terms.  The TERMS: a term is the rounded value of a few operations on
    exact products of floats (a 24 x 24 bit product is exact in double), so it is within 8 * 2^-53 of the magnitudes those
    operations saw -- for r = n.q - n.p that is |n.q| + |n.p|, not |r|: the cancellation is in the formula, and a bound
    relative to the term itself would not hold for any arithmetic."""
    rng = np.random.default_rng(5)
    m = 200
    q = rng.uniform(-2, 2, (m, 3)).astype(np.float32)
    p = (q + rng.normal(0, 0.02, (m, 3))).astype(np.float32)
    n = rng.normal(0, 1, (m, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    n[7] = np.nan                      # (a pair that stays out of the system)
    w = rng.integers(1, 4, m).astype(np.float64)
    d2 = plane_ref.d2_f32(p, q)
    sums, mag, cnt = plane_ref.plane_sums(p, q, n, w, d2)
    terms, ok = plane_ref.pair_terms(p, q, n, w, d2)
    assert cnt[0] == m and cnt[2] == m - 1 and sums[2] == sums[0] - w[7] and not ok[7] and sums[31] == 0.0
    bound = plane_ref.sums_bound(mag, cnt)
    for k in range(32):
        exact_sum = sum((Fraction(float(v)) for v in terms[:, k]), Fraction(0))
        err = abs(Fraction(float(sums[k])) - exact_sum)
        print("sum %2d: error %.3g, bound %.3g" % (k, float(err), bound[k]))
        assert err <= Fraction(float(bound[k])), k
    for i in range(m):
        W = Fraction(int(w[i]))
        exact = [Fraction(0)] * 32
        seen = [Fraction(0)] * 32
        exact[0] = seen[0] = W
        exact[1] = seen[1] = W * Fraction(float(d2[i]))
        if ok[i]:
            P, Q, N = ([Fraction(float(v)) for v in a[i]] for a in (p, q, n))
            J = [N[2] * P[1] - N[1] * P[2], N[0] * P[2] - N[2] * P[0], N[1] * P[0] - N[0] * P[1], N[0], N[1], N[2]]
            Jm = [abs(N[2] * P[1]) + abs(N[1] * P[2]), abs(N[0] * P[2]) + abs(N[2] * P[0]), abs(N[1] * P[0]) + abs(N[0] * P[1]),
                  abs(N[0]), abs(N[1]), abs(N[2])]
            r = sum(N[k] * Q[k] for k in range(3)) - sum(N[k] * P[k] for k in range(3))
            rm = sum(abs(N[k] * Q[k]) + abs(N[k] * P[k]) for k in range(3))
            exact[2] = seen[2] = W
            exact[3], seen[3] = W * r * r, W * rm * rm
            k = 4
            for a in range(6):
                for b in range(a, 6):
                    exact[k], seen[k] = W * J[a] * J[b], W * Jm[a] * Jm[b]
                    k += 1
            for a in range(6):
                exact[25 + a], seen[25 + a] = W * J[a] * r, W * Jm[a] * rm
        for k in range(32):
            assert abs(Fraction(float(terms[i, k])) - exact[k]) <= 8 * Fraction(plane_ref.U) * seen[k], (i, k)


def solve(L, sums):
    from rsreg_amd import api
    return api.plane_solve_from_sums(sums, want_rank=True)


def check_against_lstsq(L, p, q, n, expect_rank):
    sums, _, _ = plane_ref.plane_sums(p, q, n, np.ones(len(p)))
    T, rank = solve(L, sums)
    x, J = lstsq_solution(p, q, n)
    sv = np.linalg.svd(J, compute_uv=False)
    sv = sv[sv > sv[0] * 1e-9]
    cond = float((sv[0] / sv[-1]) ** 2)   # of AtA over the directions that carry data
    print("rank", rank, "cond(AtA) over the data directions %.3g" % cond)
    assert rank == expect_rank == len(sv)
    assert cond < 1e6
    Tl = plane_ref.euler_matrix(x)
    assert (np.abs(T.astype(np.float64) - Tl) <= solve_tolerance(Tl, cond)).all(), (T, Tl)
    Tr, rr = plane_ref.plane_solve(sums)
    assert rr == rank and (np.abs(T.astype(np.float64) - Tr) <= solve_tolerance(Tl, cond)).all()
    return T, x


def test_solve_three_orthogonal_walls_full_rank(L):
    rng = np.random.default_rng(11)
    q, n = walls(rng, [(0, 1.0), (1, 0.9), (2, 2.2)])
    x_true = np.array([0.01, -0.02, 0.015, 0.02, -0.01, 0.03])
    p = moved_source(q, x_true, rng)
    T, x = check_against_lstsq(L, p, q, n, 6)
    # the linearised step recovers the small motion to second order
    assert np.abs(x - x_true).max() < 2e-3


def test_solve_one_plane_rank_three(L):
    rng = np.random.default_rng(12)
    q, n = walls(rng, [(2, 2.0)])
    p = moved_source(q, np.array([0.01, -0.02, 0.0, 0.0, 0.0, 0.03]), rng)
    T, x = check_against_lstsq(L, p, q, n, 3)
    # only along the normal (tz) and about the two in-plane axes (alpha, beta): tx = ty = 0 and gamma = 0 (R[1][0] = sin(gamma)
    # cos(beta)) exactly -- the rows and columns of AtA that the plane leaves empty are exact zeros and stay so
    assert T[0, 3] == 0.0 and T[1, 3] == 0.0 and T[1, 0] == 0.0
    assert T[2, 3] != 0.0 and T[2, 0] != 0.0 and T[2, 1] != 0.0
    assert abs(x[2]) < 1e-12 and abs(x[3]) < 1e-12 and abs(x[4]) < 1e-12


def test_solve_two_parallel_planes(L):
    rng = np.random.default_rng(13)
    q, n = walls(rng, [(2, 1.0), (2, 2.0)])
    n[len(n) // 2:] *= -1          # (the far wall faces the other way: still one direction of translation)
    p = moved_source(q, np.array([0.015, 0.01, 0.0, 0.0, 0.0, -0.02]), rng)
    T, x = check_against_lstsq(L, p, q, n, 3)
    assert T[0, 3] == 0.0 and T[1, 3] == 0.0 and T[1, 0] == 0.0


def test_solve_all_zero_sums_is_identity_rank_zero(L):
    T, rank = solve(L, np.zeros(32))
    assert rank == 0 and (T == np.eye(4, dtype=np.float32)).all()
    # pairs were gated but none entered the system ([2] == 0): the identity as well
    s = np.zeros(32)
    s[0], s[1] = 10, 0.01
    T, rank = solve(L, s)
    assert rank == 0 and (T == np.eye(4, dtype=np.float32)).all()
    Tr, rr = plane_ref.plane_solve(s)
    assert rr == 0 and (Tr == np.eye(4, dtype=np.float32)).all()


def sums_from_system(A, b, count):
    s = np.zeros(32)
    s[0] = s[2] = count
    k = 4
    for i in range(6):
        for j in range(i, 6):
            s[k] = A[i, j]
            k += 1
    s[25:31] = b
    return s


def test_rank_cut_both_sides(L):
    rng = np.random.default_rng(14)
    Qm, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    x_true = np.array([0.01, -0.02, 0.005, 0.02, -0.03, 0.01])
    # an eigenvalue 1e-6 of the largest is far above the rounding of 1000 terms (6 * 1080 * 2^-53 = 7e-13): it counts as data
    lam = np.array([1.0, 0.5, 0.3, 0.2, 0.1, 1e-6]) * 1000
    A = (Qm * lam) @ Qm.T
    A = (A + A.T) / 2
    s = sums_from_system(A, A @ x_true, 1000)
    assert plane_ref.rank_cut(s) < 1e-11 * lam[0]
    T, rank = solve(L, s)
    assert rank == 6
    Te = plane_ref.euler_matrix(x_true)
    assert (np.abs(T.astype(np.float64) - Te) <= solve_tolerance(Te, 1e6)).all()
    # the same system with that direction exactly silent (built in rational steps so that the null vector is exact): rank 5,
    # and nothing moves along it
    v = np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    B = np.diag([3.0, 2.0, 0.0, 1.5, 1.0, 0.5]) * 1000
    B[0, 1] = B[1, 0] = 250.0
    B[3, 5] = B[5, 3] = -125.0
    s0 = sums_from_system(B, B @ x_true, 1000)
    T0, rank0 = solve(L, s0)
    assert rank0 == 5
    x0 = x_true - v * (v @ x_true)
    T0e = plane_ref.euler_matrix(x0)
    assert (np.abs(T0.astype(np.float64) - T0e) <= solve_tolerance(T0e, np.linalg.cond(B[np.ix_([0, 1, 3, 4, 5], [0, 1, 3, 4, 5])]))).all()
    assert T0[1, 0] == 0.0   # gamma = 0 exactly
    # an eigenvalue BELOW the cut (rounding noise of the sums) is silent as well
    lam2 = lam.copy()
    lam2[5] = 1e-14 * lam[0]
    A2 = (Qm * lam2) @ Qm.T
    A2 = (A2 + A2.T) / 2
    _, rank2 = solve(L, sums_from_system(A2, A2 @ x_true, 1000))
    assert rank2 == 5
    assert plane_ref.plane_solve(sums_from_system(A2, A2 @ x_true, 1000))[1] == 5


def test_brute_and_tree_search_agree():
    rng = np.random.default_rng(15)
    t = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    t[100] = t[7]                      # exact copies: the lowest index wins
    t[50] = np.nan
    q = np.concatenate([t[:400] + rng.normal(0, 0.01, (400, 3)).astype(np.float32), t[7:8], [[np.inf, 0, 0]]]).astype(np.float32)
    ib, db = plane_ref.nearest_brute(q, t)
    it, dt = plane_ref.filters_ref.nearest(q, t)
    assert (ib == it).all() and (db == dt).all() and ib[400] == 7 and ib[401] == -1


@pytest.fixture(scope="module")
def bench_pair(rs):
    from rsreg_amd import synth
    import filters_ref
    import normals_ref
    tgt = filters_ref.xyz(synth.render_frame(0, "50k", "bench"))
    src = filters_ref.xyz(synth.render_frame(1, "50k", "bench"))
    nrm = normals_ref.normals(tgt, 10).normal
    return src, tgt, nrm, synth.ground_truth(1, 0, "bench")


def test_reference_loop_plane_beats_point_on_bench_pair(bench_pair):
    """The condition on the fixture that tests/test_plane_icp_gpu.py relies on: render_frame(0 / 1, "50k", "bench") from the
    identity, 5 cm gate, 10 iterations."""
    src, tgt, nrm, truth = bench_pair
    plane = plane_ref.plane_icp(src, tgt, nrm, None, 10, 0.05, truth)
    point = plane_ref.plane_icp(src, tgt, nrm, None, 10, 0.05, truth, point_to_plane=False)
    print("point-to-plane |T - truth|_F per iteration:", ["%.4g" % e for e in plane.errors])
    print("point-to-point |T - truth|_F per iteration:", ["%.4g" % e for e in point.errors])
    assert plane.iterations == point.iterations == 10
    assert plane.errors[-1] <= point.errors[-1]
    assert np.isfinite(plane.T).all()


def test_abi_estimation_field_and_symbols(L):
    assert L.IcpParams.estimation.offset == 12 and L.IcpParams.estimation.size == 4
    assert C.sizeof(L.IcpParams) == 64 and L.lib().rsreg_version() == 4
    assert L.NUM_PLANE_SUMS == 32
    from rsreg_amd import api
    for reference in (False, True):
        assert api.icp_params(reference=reference).estimation == L.ESTIMATION_SVD
    for name in ("rsreg_icp_set_target_normals", "rsreg_icp_set_target_normals_cloud", "rsreg_icp_plane_sums", "rsreg_icp_update_plane",
                 "rsreg_icp_plane_sums_last", "rsreg_plane_solve_from_sums"):
        assert name in L.EXPORTS and getattr(L.lib(), name) is not None
    assert api.POINT_NORMAL_DTYPE.itemsize == 48 and api.POINT_NORMAL_DTYPE.fields["normal_x"][1] == 16
    assert api.IterativeClosestPointWithNormals.__mro__[1] is api.IterativeClosestPoint
    # NULL arguments are refused, not dereferenced
    assert L.lib().rsreg_plane_solve_from_sums(None, None, None) == L.RSREG_ERR_INVALID_ARG
