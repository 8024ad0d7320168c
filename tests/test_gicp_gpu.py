"""GeneralizedIterativeClosestPoint on the GPU (rsreg_cloud_gicp_covariances: k_gicp_cov; rsreg_gicp_*: k_gicp_mahalanobis,
k_gicp_reduce, the host loop) against tests/gicp_ref.py, the numpy restatement of include/rsreg.h.

Covariances.  The reference is fed the engine's own neighbour indices (rsreg_cloud_knn, itself held bit-equal to its reference by
tests/test_normals_gpu.py).  Where the eigen-gap ratio (l1 - l0) / l2 of the reference covariance is at least 1e-3 -- the cut of
the normals test -- that test allows the normal an angle of h = 2^-22 rad to +-n_ref.  Carried through C' = I - s n n^T (s = 1 - eps
< 1): with d = n - n_ref (or n + n_ref; n n^T does not see the sign), |d| = 2 sin(angle / 2) <= h, and
    |n_a n_b - r_a r_b| = |n_a d_b + d_a r_b| <= |d_b| + |d_a| <= 2 h          (|n_a|, |r_b| <= 1)
so every entry of C' is within 2 s h of the reference's, plus the three roundings of the formula (3 * 2^-53): COV_TOL = 2^-21.
Everywhere, gap or none, C' has the eigenvalues (eps, 1, 1) of a unit n to 1e-12; records whose neighbours coincide (trace 0) and
non-finite records are exact.

Sums.  The 32 sums at X = I and at a non-trivial X against the reference's terms of the same pairs: a sum of N terms, however
ordered, is within (N + 16) * 2^-53 * sum|term| of the exact one (the bound of the plane test); [0] and [1] bit-equal to
rsreg_icp_sums [0] and [16] of the same search on a second context.

Whole alignments at tight epsilons (1e-7), where engine and reference sit at the fixed point: within 1e-4 Frobenius of the
reference's transform (tests/test_gicp_cpu.py shows the cases move by less than 1e-5 under a 1e-12 perturbation of every sum),
within the CPU-pinned margin of the truth; align, align_cloud and the step-wise form give the same bytes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import filters_ref
import fitness_ref
import gicp_cases as GC
import gicp_ref as G
import plane_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GATE = 0.05
GAP_CUT = 1e-3
COV_TOL = 2.0 ** -21
EPS = 1e-3


@pytest.fixture(scope="module")
def api():
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    return api


@pytest.fixture(scope="module")
def ctxs(api):
    return api.Context(0), api.Context(0)


@pytest.fixture(scope="module")
def walls():
    tgt, nrm = PC.three_walls(2000)
    return tgt, nrm, GC.plane_covariances(nrm)


def _unit(n, seed):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _uniform(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * np.array([2.0, 1.5, 0.7]) + np.array([-1.0, -0.5, 0.4])).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ covariances
def _check_covariances(api, ctx, xyz, k, eps=EPS, dev=None, label=""):
    dev = dev or api.DeviceCloud(PC.cloud(xyz), ctx=ctx)
    cov, dense = dev.gicp_covariances(k, eps)
    idx, _ = dev.knn(k)
    ref = G.covariances(xyz, k, eps, idx=idx)
    fin = np.isfinite(xyz).all(axis=1)
    assert (ref.finite == fin).all()
    assert cov.shape == (len(xyz), 6) and np.isnan(cov[~fin]).all() and np.isfinite(cov[fin]).all()
    assert dense is False                                   # (PC.cloud hands the records in as not dense: the result never claims more)
    flat = fin & (np.trace(ref.C, axis1=1, axis2=2) == 0)
    assert cov[flat].tobytes() == ref.cov[flat].tobytes()
    use = fin & (ref.gap >= GAP_CUT)
    err = float(np.abs(cov[use] - ref.cov[use]).max()) if use.any() else 0.0
    w = np.linalg.eigvalsh(G.full(cov[fin]))
    print("%s k=%d n=%d: %d records above the gap cut, max |C' - ref| = %.3g, eigenvalues off by %.3g"
          % (label, k, len(xyz), int(use.sum()), err, float(np.abs(w - np.array([eps, 1.0, 1.0])).max())))
    assert err <= COV_TOL
    assert np.abs(w - np.array([eps, 1.0, 1.0])).max() < 1e-12
    return cov, ref


@pytest.mark.parametrize("k", [4, 20, 64])
def test_covariances_on_small_and_odd_clouds(api, ctxs, k):
    for n in sorted({k, k + 1, 64, 65, 300}):
        if n >= k:
            _check_covariances(api, ctxs[0], _uniform(n, 10 * k + n), k, label="uniform")


def test_covariances_on_a_plane_a_line_a_pile_and_non_finite_records(api, ctxs):
    rng = np.random.default_rng(21)
    plane = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    plane[:, 2] = 1.5
    cov, ref = _check_covariances(api, ctxs[0], plane, 20, label="plane")
    assert (ref.gap >= GAP_CUT).all() and np.abs(cov - np.array([1, 0, 0, 1, 0, EPS])).max() <= COV_TOL
    line = np.zeros((200, 3), np.float32)
    line[:, 0] = np.linspace(-1, 1, 200)
    line[:, 1] = 0.25
    line[:, 2] = 2.0
    cov, ref = _check_covariances(api, ctxs[0], line, 8, label="line")      # (l0 = l1: n is any unit vector across the line)
    assert np.abs(cov[:, 0] - 1.0).max() < 1e-9                               # ... so C'_xx = 1 - s * n_x^2 with n_x = 0
    pile = np.concatenate([np.repeat(np.array([[0.5, -0.25, 1.0]], np.float32), 30, axis=0), _uniform(200, 22)])
    pile[100] = np.nan
    pile[101, 1] = np.inf
    pile[102] = (-np.inf, np.nan, 0)
    cov, ref = _check_covariances(api, ctxs[0], pile, 20, label="pile, NaN, Inf")
    assert (cov[:30] == np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0 - (1.0 - EPS) * 1.0])).all()
    assert np.isnan(cov[100:103]).all()
    # (a cloud that says it is dense and is: the result says so too; one NaN record: not dense)
    dense = api.DeviceCloud(api.NormalCloud(PC.cloud(plane).points, len(plane), 1, True), ctx=ctxs[0])
    assert dense.gicp_covariances(20, EPS)[1] is True
    holed = PC.cloud(pile)
    holed.is_dense = True
    assert api.DeviceCloud(holed, ctx=ctxs[0]).gicp_covariances(20, EPS)[1] is False


def test_covariances_record_strides_and_contexts(api, ctxs):
    xyz = _uniform(300, 23)
    want, _ = _check_covariances(api, ctxs[0], xyz, 20, label="stride 32")
    rec12 = np.ascontiguousarray(xyz).view(np.dtype((np.void, 12))).reshape(-1)
    rec48 = np.zeros(len(xyz), api.POINT_NORMAL_DTYPE)
    for name, col in zip("xyz", xyz.T):
        rec48[name] = col
    rec48["normal_x"] = 7.0
    for rec in (rec12, rec48):
        dev = api.DeviceCloud(api.NormalCloud(rec, len(rec), 1, False), ctx=ctxs[0])
        assert dev.info()[1] == rec.dtype.itemsize
        assert dev.gicp_covariances(20, EPS)[0].tobytes() == want.tobytes()
    other = api.DeviceCloud(PC.cloud(xyz), ctx=ctxs[1])
    assert other.gicp_covariances(20, EPS)[0].tobytes() == want.tobytes()
    for k in (3, 65, 0):
        with pytest.raises(Exception) as e:
            other.gicp_covariances(k, EPS)
        assert e.value.status == -1 and "between 4 and 64" in str(e.value)
    with pytest.raises(Exception) as e:
        api.DeviceCloud(PC.cloud(xyz[:10]), ctx=ctxs[1]).gicp_covariances(20, EPS)
    assert e.value.status == -1


# ------------------------------------------------------------------------------------------------------------ sums
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 127, 128, 129, 1000])
def test_sums_at_tile_and_wave_edges(api, ctxs, walls, n):
    tgt, _, cov_t = walls
    src = PC.source_near(tgt, n, seed=100 + n)
    GC.stepwise_check(api, src, tgt, G.regularised(_unit(n, n), EPS), cov_t, ctx=ctxs[0], ctx2=ctxs[1], label="n=%d" % n)


def test_sums_under_a_guess(api, ctxs, walls):
    tgt, _, cov_t = walls
    guess = PC.plane_ref.euler_matrix(np.array([0.004, -0.006, 0.005, 0.006, -0.004, 0.008]))
    src = PC.source_near(tgt, 700, seed=31)
    GC.stepwise_check(api, src, tgt, G.regularised(_unit(700, 32), EPS), cov_t, guess=guess, ctx=ctxs[0], ctx2=ctxs[1], label="guess")


def test_merged_copies_carry_their_weight(api, ctxs, walls):
    """70 000 source records of which 10 000 are exact copies (with their covariance, bit for bit): above 65 536 records the
    engine merges copies, W = cur.w."""
    tgt, _, cov_t = walls
    src = PC.source_near(tgt, 60_000, seed=7)
    cov = G.regularised(_unit(60_000, 9), EPS)
    rng = np.random.default_rng(8)
    pick = rng.integers(0, 60_000, 10_000)
    order = rng.permutation(70_000)
    src = np.concatenate([src, src[pick]])[order]
    cov = np.concatenate([cov, cov[pick]])[order]
    s_i, _, k, _, g = GC.stepwise_check(api, src, tgt, cov, cov_t, ctx=ctxs[0], ctx2=ctxs[1], label="70k with copies")
    assert 60_000 <= g.grid_info().n_source_distinct < 70_000 and s_i[0] == len(k) > 60_000


def test_non_finite_records_and_points_outside_the_gate(api, ctxs, walls):
    tgt, _, cov_t = walls
    src = PC.source_near(tgt, 500, seed=11)
    src[3] = np.nan
    src[10, 1] = np.inf
    src[77] = (-np.inf, np.nan, 0)
    src[100:160] += np.float32(0.5)        # far outside the 5 cm gate
    s_i, _, _, _, _ = GC.stepwise_check(api, src, tgt, G.regularised(_unit(500, 12), EPS), cov_t, ctx=ctxs[0], ctx2=ctxs[1], label="NaN, Inf, unmatched")
    assert 4 <= s_i[0] <= 500 - 3 - 60 + 5


def test_every_third_target_covariance_nan(api, ctxs, walls):
    tgt, _, cov_t = walls
    cov_t = cov_t.copy()
    cov_t[::3, 0] = np.nan                 # (every record of the wall x = -1: that wall drops out of the system)
    cov_t[1::30, 5] = np.inf
    cov_s = G.regularised(_unit(1000, 13), EPS)
    cov_s[5] = np.nan
    s_i, s_x, _, ok, _ = GC.stepwise_check(api, PC.source_near(tgt, 1000, seed=12), tgt, cov_s, cov_t, ctx=ctxs[0], ctx2=ctxs[1],
                                           label="every third target covariance NaN")
    assert 0 < s_i[2] == ok.sum() < s_i[0] and s_x[2] == s_i[2]


@pytest.mark.parametrize("env,kind", [({"RSREG_FORCE_HASH": "1"}, 0), ({}, 1)], ids=["brick-hash", "dense-grid"])
def test_both_index_kinds(env, kind):
    e = dict(os.environ, GICP_CASE_INDEX_KIND=str(kind), PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gicp_cases.py"), "walls_index_kind"], cwd=ROOT, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "gicp case ok" in r.stdout, r.stdout[-3000:]


def test_one_plane_target_and_a_source_on_an_axis(api, ctxs):
    """A one-plane target.  Its pairs all weigh the plane's normal 1 / (2 eps) and the plane's own directions 1 / 2: the system
    keeps its full rank, and the alignment stays finite and rigid.  The rank drops where the DATA is silent: source points on the
    x axis say nothing about a rotation about it -- row and column 0 of H and b_0 are exact zeros, the solve uses five
    directions and the unobserved angle does not move."""
    rng = np.random.default_rng(31)
    tgt = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    tgt[:, 2] = 2.0
    nz = np.zeros((3000, 3))
    nz[:, 2] = 1.0
    cov = GC.plane_covariances(nz)
    src = tgt[:1500].copy()
    src[:, 2] += np.float32(0.02)
    src[:, 0] += np.float32(0.003)
    g = GC.make_gicp(api, ctxs[0], src, tgt, cov[:1500], cov, GATE, **GC.TIGHT)
    g.align()
    T = g.getFinalTransformation().astype(np.float64)
    assert np.isfinite(T).all() and g.result.converged and g.result.rank_last == 6
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(T[:3, :3]) - 1) < 1e-6
    assert (T[3] == (0, 0, 0, 1)).all() and abs(T[2, 3] + 0.02) < 1e-4 and abs(T[0, 3] + 0.003) < 1e-3
    flat = rng.uniform(-1, 1, (12_000, 3)).astype(np.float32)   # (dense enough for every source point to have a match within the gate)
    flat[:, 2] = -0.01
    axis = np.zeros((60, 3), np.float32)
    axis[:, 0] = np.linspace(-0.9, 0.9, 60)
    g = GC.make_gicp(api, ctxs[0], axis, flat, cov[:60], np.tile(cov[:1], (12_000, 1)), GATE)
    g.begin()
    g.search()
    S = g.gicp_sums()
    x, D, rank = api.gicp_step_from_sums(S)
    H, b = PC.plane_ref.system(S)
    assert S[2] == 60 and not H[0].any() and b[0] == 0 and rank == 5 and x[0] == 0.0 and np.isfinite(x).all()
    assert abs(x[5] + 0.01) < 1e-6 and D[2, 1] == 0.0                          # (cos(beta) sin(alpha): no rotation about x in the increment)
    g.update(None, S, 0)
    g.end()
    assert g.result.rank_last == 5 and np.isfinite(np.array(g.result.transform)).all()


# ------------------------------------------------------------------------------------------------------------ whole alignments
@pytest.mark.parametrize("name", GC.ALIGN_CASES)
def test_whole_alignment_matches_the_reference(api, name):
    c = GC.align_case(name)
    ref = GC.align_reference(name)
    ctx = api.Context(0)
    tight = dict(GC.TIGHT, max_inner_iterations=c.prm.max_inner_iterations)
    g = GC.make_gicp(api, ctx, c.src, c.tgt, c.cov_s, c.cov_t, c.prm.max_correspondence_distance, **tight)
    out = g.align()
    T = g.getFinalTransformation()
    err = float(np.linalg.norm(T.astype(np.float64) - ref.T.astype(np.float64)))
    truth = float(np.linalg.norm(T.astype(np.float64) - c.truth))
    print("%s: |T - T_ref|_F = %.3g, |T - truth|_F = %.3g, iterations %d / %d, inner evaluations %d / %d, pairs %d / %d"
          % (name, err, truth, g.result.iterations, ref.iterations, g.result.inner_evaluations, ref.inner_evaluations,
             g.result.n_correspondences, ref.n_correspondences))
    assert err < 1e-4 and truth <= GC.TRUTH_MARGIN[name]
    assert g.hasConverged() and api.CONV_STATES[g.result.state] == "TRANSFORM"
    assert g.result.n_correspondences == ref.n_correspondences
    assert g.result.mse == g.result.sums_last[1] / g.result.sums_last[0]
    whole = (bytes(g.result.transform), bytes(g.result.sums_last), g.result.iterations, g.result.inner_evaluations)
    want = api.transformPointCloud(PC.cloud(c.src), T, ctx=ctx)
    for k in "xyz":
        np.testing.assert_array_equal(out.points[k], want.points[k])
    # getFitnessScore after it
    score, count = g.fitnessScore(GATE * GATE)
    ws, wn = fitness_ref.fitness(filters_ref.xyz(want), c.tgt, GATE * GATE, valid=fitness_ref.finite_rows(c.src))
    assert count == wn and abs(score - ws) <= 1e-12 * ws
    # the same alignment on device clouds (the covariances from device clouds too), and step by step from here
    dev_s, dev_t = api.DeviceCloud(PC.cloud(c.src), ctx=ctx), api.DeviceCloud(PC.cloud(c.tgt), ctx=ctx)
    cs = api.DeviceCloud(api.NormalCloud(np.ascontiguousarray(c.cov_s).view(np.dtype((np.void, 48))).reshape(-1), len(c.cov_s), 1, True), ctx=ctx)
    ct = api.DeviceCloud(api.NormalCloud(np.ascontiguousarray(c.cov_t).view(np.dtype((np.void, 48))).reshape(-1), len(c.cov_t), 1, True), ctx=ctx)
    gd = GC.make_gicp(api, ctx, dev_s, dev_t, cs, ct, c.prm.max_correspondence_distance, **tight)
    got = gd.align().download()
    assert (bytes(gd.result.transform), bytes(gd.result.sums_last), gd.result.iterations, gd.result.inner_evaluations) == whole
    for k in "xyz":
        np.testing.assert_array_equal(got.points[k], out.points[k])
    gs = GC.make_gicp(api, api.Context(0), c.src, c.tgt, c.cov_s, c.cov_t, c.prm.max_correspondence_distance, **tight)
    res = GC.engine_stepwise_align(api, gs)
    assert (bytes(res.transform), bytes(res.sums_last), res.iterations, res.inner_evaluations) == whole


def test_pcl_defaults_once(api):
    """PCL's defaults, the covariances computed by the class itself (k = 20, epsilon = 1e-3) as PCL does when none are given."""
    c = GC.align_case("walls5k")
    g = api.GeneralizedIterativeClosestPoint(api.Context(0, profiling=True))
    g.setInputSource(PC.cloud(c.src))
    g.setInputTarget(PC.cloud(c.tgt))
    g.align()
    r = g.result
    # (a profiling context: the device-time breakdown the ICP result has)
    assert r.ms_nn > 0 and r.ms_reduce > 0 and r.ms_total == r.ms_nn + r.ms_reduce + r.ms_transform and r.n_nn_launches == r.iterations
    T = g.getFinalTransformation().astype(np.float64)
    print("defaults: %d iterations, %d inner evaluations, |T - truth|_F %.3g" % (r.iterations, r.inner_evaluations, np.linalg.norm(T - c.truth)))
    assert g.hasConverged() and 1 <= r.iterations <= 200 and r.inner_evaluations <= 20 * r.iterations
    assert r.n_correspondences == 5000 and np.linalg.norm(T - c.truth) < 0.1 * np.linalg.norm(np.eye(4) - c.truth)


# ------------------------------------------------------------------------------------------------------------ error paths
def test_error_paths(api, walls):
    from rsreg_amd import lib as L
    import ctypes as C
    tgt, _, cov_t = walls
    src = PC.source_near(tgt, 200, seed=41)
    cov_s = G.regularised(_unit(200, 42), EPS)
    ctx = api.Context(0)
    lib = L.lib()
    t, s = PC.cloud(tgt).points, PC.cloud(src).points
    prm = api.gicp_params(max_correspondence_distance=GATE)
    res = L.GicpResult()
    sums = np.zeros(32)
    assert lib.rsreg_gicp_set_source_covariances(ctx.h, cov_s.ctypes.data, 200, 48) == -8     # RSREG_ERR_NO_SOURCE
    assert lib.rsreg_gicp_set_target_covariances(ctx.h, cov_t.ctypes.data, 2000, 48) == -5    # RSREG_ERR_NO_TARGET
    assert lib.rsreg_icp_set_source(ctx.h, s.ctypes.data, len(s), 32, 0) == 0
    assert lib.rsreg_icp_set_target(ctx.h, t.ctypes.data, len(t), 32, 0, GATE) == 0
    assert lib.rsreg_gicp_begin(ctx.h, None, C.byref(prm)) == L.RSREG_ERR_STATE               # no covariances
    assert lib.rsreg_gicp_align(ctx.h, None, C.byref(prm), C.byref(res), None, 0) == L.RSREG_ERR_STATE
    assert lib.rsreg_gicp_set_source_covariances(ctx.h, cov_s.ctypes.data, 199, 48) == L.RSREG_ERR_INVALID_ARG
    assert lib.rsreg_gicp_set_target_covariances(ctx.h, cov_t.ctypes.data, 2001, 48) == L.RSREG_ERR_INVALID_ARG
    assert lib.rsreg_gicp_set_source_covariances(ctx.h, cov_s.ctypes.data, 200, 40) == L.RSREG_ERR_INVALID_ARG
    assert lib.rsreg_gicp_set_source_covariances(ctx.h, cov_s.ctypes.data, 200, 48) == 0
    assert lib.rsreg_gicp_begin(ctx.h, None, C.byref(prm)) == L.RSREG_ERR_STATE               # only one of the two sets
    assert lib.rsreg_gicp_set_target_covariances(ctx.h, cov_t.ctypes.data, 2000, 48) == 0
    assert lib.rsreg_gicp_sums(ctx.h, None, sums.ctypes.data) == L.RSREG_ERR_STATE            # before begin
    assert lib.rsreg_gicp_begin(ctx.h, None, C.byref(prm)) == 0
    assert lib.rsreg_gicp_sums(ctx.h, None, sums.ctypes.data) == L.RSREG_ERR_STATE            # before the search
    assert lib.rsreg_gicp_search(ctx.h, None, None) == 0
    assert lib.rsreg_gicp_sums(ctx.h, None, sums.ctypes.data) == 0 and sums[0] >= 4
    assert lib.rsreg_gicp_end(ctx.h, C.byref(res), None, 0) == 0
    assert lib.rsreg_gicp_end(ctx.h, C.byref(res), None, 0) == L.RSREG_ERR_STATE
    bad = api.gicp_params(max_correspondence_distance=GATE, max_inner_iterations=-1)
    assert lib.rsreg_gicp_begin(ctx.h, None, C.byref(bad)) == L.RSREG_ERR_INVALID_ARG
    wide = api.gicp_params(max_correspondence_distance=2 * GATE)                              # wider than the index was built for
    assert lib.rsreg_gicp_begin(ctx.h, None, C.byref(wide)) == L.RSREG_ERR_INVALID_ARG
    assert lib.rsreg_gicp_align(ctx.h, None, C.byref(prm), C.byref(res), None, 0) == 0 and res.converged == 1
    # a new target drops the target's covariances, a new source the source's
    assert lib.rsreg_icp_set_target(ctx.h, t.ctypes.data, len(t), 32, 0, GATE) == 0
    assert lib.rsreg_gicp_begin(ctx.h, None, C.byref(prm)) == L.RSREG_ERR_STATE
    assert lib.rsreg_gicp_set_target_covariances(ctx.h, cov_t.ctypes.data, 2000, 48) == 0
    assert lib.rsreg_gicp_begin(ctx.h, None, C.byref(prm)) == 0
    assert lib.rsreg_icp_set_source(ctx.h, s.ctypes.data, len(s), 32, 0) == 0
    assert lib.rsreg_gicp_search(ctx.h, None, None) == L.RSREG_ERR_STATE                      # (and the alignment that was under way is over)
    assert lib.rsreg_gicp_begin(ctx.h, None, C.byref(prm)) == L.RSREG_ERR_STATE
    assert lib.rsreg_gicp_set_source_covariances(ctx.h, cov_s.ctypes.data, 200, 48) == 0
    assert lib.rsreg_gicp_begin(ctx.h, None, C.byref(prm)) == 0
    assert lib.rsreg_gicp_end(ctx.h, None, None, 0) == 0
    # GICP is no third estimation of rsreg_icp_begin
    assert lib.rsreg_icp_begin(ctx.h, None, C.byref(api.icp_params(max_correspondence_distance=GATE, estimation=2))) == L.RSREG_ERR_INVALID_ARG
    # and the point-to-point path of the same context still runs
    icp = api.icp_params(max_correspondence_distance=GATE)
    ires = L.IcpResult()
    assert lib.rsreg_icp_align(ctx.h, None, C.byref(icp), C.byref(ires), None, 0) == 0 and ires.n_correspondences >= 4


TWO_RANKS = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
from rsreg_amd import api, lib
import gicp_cases as GC
import gicp_ref as G
import plane_cases as PC
tgt, nrm = PC.three_walls(2000)
src = PC.source_near(tgt, 300, seed=5)
two = api.Context(0)
assert lib.lib().rsreg_diag_set_nranks(two.h, 2) == 0
g = GC.make_gicp(api, two, src, tgt, GC.plane_covariances(nrm[:300]), GC.plane_covariances(nrm), 0.05)
for step in ("align", "begin"):
    try:
        g.begin() if step == "begin" else g.align()
    except lib.RsregError as e:
        assert e.status == -1 and "more than one rank" in str(e), e
    else:
        raise AssertionError("GICP accepted on two ranks: " + step)
one = api.Context(0)
one.comm_init(api.comm_unique_id(), 0, 1)
a = GC.make_gicp(api, one, src, tgt, GC.plane_covariances(nrm[:300]), GC.plane_covariances(nrm), 0.05)
b = GC.make_gicp(api, api.Context(0), src, tgt, GC.plane_covariances(nrm[:300]), GC.plane_covariances(nrm), 0.05)
a.align()
b.align()
assert bytes(a.result.transform) == bytes(b.result.transform) and bytes(a.result.sums_last) == bytes(b.result.sums_last)
assert lib.lib().rsreg_comm_destroy(one.h) == 0
print("REFUSED OK")
'''


def test_two_ranks_are_refused():
    """A communicator with more than one rank: RSREG_ERR_INVALID_ARG with a message.  Two ranks need two GPUs; the context counts
    itself one of two through the hook of the diagnostic build, in a child process (tests/test_sharded_gpu.py does the same for the
    correspondence filters).  A one-rank communicator runs and gives the plain context's bytes."""
    from rsreg_amd import lib
    lib.build_diag()
    env = dict(os.environ, RSREG_DIAG="1")
    env.pop("RSREG_SO", None)
    r = subprocess.run([sys.executable, "-c", TWO_RANKS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0 and "REFUSED OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
