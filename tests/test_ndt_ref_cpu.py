"""The slow NDT of tests/ndt_ref.py shown right before anything is measured against it: against the numpy golden vectors of
`ndt_small` (the only independent check NDT had), against the C oracle at four poses, and every case of tests/ndt_cases.py
through the C oracle.  Derivatives are compared with the reference at x' in float32 (what the oracle evaluates), on the
oracle's own f64 table (which check_grid judges), to ndt_ref.F64_BAR of each sum's fscale: f64 rounding alone, about 1e-11 of its scale.
The gap between float32 and exact x' that ndt_ref.DERIV_BAR stands for is measured again here.

What this file found: the row h_ang_d1 of PCL's angle table ends in +sin(ay) where d2(Rx)/d(ay)^2 has -sin(ay); engine and
oracle restate PCL, the reference reproduces it as a named switch (ndt_ref module docstring), and
test_pcl_d1_is_the_only_departure_from_the_derivative pins that nothing else differs."""
import mpmath as mp
import numpy as np
import pytest

import ndt_cases as K
import ndt_ref as R
from ndt_ref import check_grid

GRID = {c["name"]: c for c in K.grid_cases()}
PASS = {c["name"]: c for c in K.pass_cases()}


def _rec(xyz):
    return np.ascontiguousarray(np.c_[np.asarray(xyz, np.float32).reshape(-1, 3), np.ones(len(xyz), np.float32)])


@pytest.fixture(scope="module")
def grids():
    memo = {}

    def get(c):
        if c["name"] not in memo:
            memo[c["name"]] = R.grid(c["tgt"], c["res"])
        return memo[c["name"]]
    return get


def _oracle(orc, tgt, res, mode):
    o = orc.NdtOracle()
    o.set_centroid_mode(mode)   # 1: the rounded f64 mean, 0: PCL's float running sum
    o.set_target(_rec(tgt), res)
    return o


@pytest.fixture(scope="module")
def small_grid(golden):
    return R.grid(golden("ndt_small")["tgt"][:, :3], 1.0)


def _against_oracle(o, ref, src, res, pose, params):
    """The oracle's 28 sums against the reference at x' in float32 on the oracle's own table: f64 rounding alone."""
    d = R.derivatives(src, R.with_table(ref, o.voxels()[0]), res, pose, xprime="f32")
    got = R.pack(*o.derivatives(_rec(src), np.asarray(pose, np.float64), params))
    err, bound = np.abs(got - d["sums"]), R.F64_BAR * d["fscale"]
    print("worst err / bound %.3g, bound / scale %.3g" % (np.max(err / np.maximum(bound, 1e-300)), np.max(bound / np.maximum(d["scale"], 1e-300))))
    assert (err <= bound).all(), err / np.maximum(d["scale"], 1e-300)
    return d, got


def test_reference_grid_matches_the_golden_vectors(golden, small_grid):
    g = golden("ndt_small")
    ref = small_grid
    m, c = R.as_table(ref)
    np.testing.assert_array_equal(c, g["vox_n"])
    np.testing.assert_allclose(m[:, 0:3], g["vox_mean"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(m[:, 3:12].reshape(-1, 3, 3), g["vox_cov"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(m[:, 12:21].reshape(-1, 3, 3), g["vox_icov"], rtol=1e-7, atol=1e-9)
    d = R.derivatives(g["src"][:, :3], ref, 1.0, g["pose"], xprime="f32")
    assert abs(d["sums"][0] - g["score"][0]) < 1e-6 * abs(g["score"][0])
    score, grad, hess = R.unpack(d["sums"])
    np.testing.assert_allclose(grad, g["grad_fd"], rtol=5e-4, atol=0.5)
    np.testing.assert_allclose(hess, g["hess_fd"], rtol=2e-3, atol=np.abs(g["hess_fd"]).max() * 2e-4)


@pytest.mark.parametrize("pose", ["golden", "general", "snap_a", "snap_b"])
def test_reference_derivatives_match_the_oracle(orc, golden, small_grid, pose):
    g = golden("ndt_small")
    tgt, src = g["tgt"][:, :3], g["src"][:256, :3]
    p = np.asarray(g["pose"] if pose == "golden" else K.POSES[pose], np.float64)
    d, _ = _against_oracle(_oracle(orc, tgt, 1.0, 1), small_grid, src, 1.0, p, orc.NdtParams.reference())
    assert d["pairs"] > 100 and d["margin"] > 1e-5


@pytest.mark.parametrize("name", list(GRID))
def test_every_grid_case_through_the_oracle(orc, grids, name):
    c = GRID[name]
    g = grids(c)
    e = c["expect"]
    for k in ("div", "n_leaves", "occupied", "n_finite"):
        if k in e:
            assert g[k] == e[k], (k, g[k], e[k])
    if "kept" in e:
        assert len(g["vox"]) == e["kept"]
    if "counts" in e:
        assert sorted(v["n"] for v in g["vox"]) == sorted(e["counts"])
    for mode in (1, 0):
        o = _oracle(orc, c["tgt"], c["res"], mode)
        m, cnt = o.voxels()
        check_grid(c, g, m, cnt, o.centroids(), pcl_mode=(mode == 0))


def test_branch_selectors_of_the_grid_cases(grids):
    """The host-visible values that select a branch of rsreg_ndt_set_target_device, from the reference's own numbers."""
    n_leaves = {n: grids(GRID[n])["n_leaves"] for n in ("keys32_div1290", "keys64_div1291", "keys64_far", "few_leaves_fewer_points")}
    assert n_leaves["keys32_div1290"] == 1290 ** 3 < 0x7fffffff <= 1291 ** 3 == n_leaves["keys64_div1291"] < n_leaves["keys64_far"]
    few = grids(GRID["few_leaves_fewer_points"])
    assert few["n_finite"] < few["n_leaves"] <= 256 and few["occupied"] < few["n_finite"]
    assert grids(GRID["occupied_2048"])["occupied"] == 2048 and grids(GRID["occupied_2049"])["occupied"] == 2049
    for n in ("occupied_2048", "occupied_2049"):
        cnt = grids(GRID[n])["occupied_counts"]
        assert set(range(1, 16)) <= set(cnt) and {256, 257} <= set(cnt)       # dropped leaves of 1..5 among kept ones of 6..15
    assert {255, 256, 257, 4095, 4096, 4097, 6, 15} <= set(grids(GRID["runs_on_the_block_stride"])["occupied_counts"])
    assert sorted(set(grids(GRID["min_points_interleaved"])["occupied_counts"])) == [1, 2, 3, 4, 5, 6, 7, 8]
    e = grids(GRID["binning_edges"])
    # the boundary points did fall on both sides: some products round up to k, some stay under it
    assert len(set(e["occupied_counts"])) > 1 and e["occupied_counts"].sum() == GRID["binning_edges"]["expect"]["n_finite"]
    far = grids(GRID["voxel_far_from_origin"])["vox"][0]
    assert float(far["sxx"].max() / far["n"]) > 1e7 * float(far["lam"][2])      # far from the origin relative to its spread
    assert [grids(GRID[n])["vox"][0]["floored"] for n in ("flat_exact", "collinear_exact", "isotropic")] == [True, True, False]
    assert float(grids(GRID["coincident"])["vox"][0]["lam"][2]) == 0.0


@pytest.fixture(scope="module")
def pass_refs(grids):
    memo = {}

    def get(c, xprime):
        k = (c["name"], xprime)
        if k not in memo:
            memo[k] = R.derivatives(c["src"], grids(c), c["res"], c["pose"], xprime=xprime)
        return memo[k]
    return get


@pytest.mark.parametrize("name", list(PASS))
def test_every_pass_case_through_the_oracle(orc, grids, pass_refs, name):
    c = PASS[name]
    g = grids(c)
    d = pass_refs(c, "f32")
    assert (len(c["src"]), len(g["vox"])) == (c["expect"]["n"], c["expect"]["n_vox"])
    if "pairs" in c["expect"]:
        assert d["pairs"] == c["expect"]["pairs"]
    assert d["margin"] > 1e-3      # no pair near enough to the radius for a last bit of the pose matrix to move it
    o = _oracle(orc, c["tgt"], c["res"], 1)
    m, cnt = o.voxels()
    check_grid({"name": name, "degenerate": name == "zero_inverse"}, g, m, cnt, o.centroids(), pcl_mode=False)
    if len(c["src"]):
        _against_oracle(o, g, c["src"], c["res"], c["pose"], orc.NdtParams.reference())
    if name == "zero_inverse":
        zero = [j for j, v in enumerate(g["vox"]) if float(v["lam"][2]) == 0.0]
        assert len(zero) == 1 and d["inc"][:, zero[0]].sum() == 20      # pairs with e = 1 exactly: score only


def test_f32_gap_behind_the_bar(pass_refs):
    """DERIV_F32_GAP again: reference at x' in float32 against reference at x' exact, every pass case, each sum by its scale."""
    worst, by = 0.0, None
    for c in PASS.values():
        a, b = pass_refs(c, "f32"), pass_refs(c, "exact")
        np.testing.assert_array_equal(a["inc"], b["inc"])
        gap = float(np.max(np.abs(a["sums"] - b["sums"]) / np.maximum(b["scale"], 1e-300)))
        if gap > worst:
            worst, by = gap, c["name"]
    print("measured gap %.3e (%s); recorded %.3e" % (worst, by, R.DERIV_F32_GAP))
    assert 0.5 * R.DERIV_F32_GAP < worst <= R.DERIV_F32_GAP and R.DERIV_BAR == 4 * R.DERIV_F32_GAP


def test_point_derivatives_are_the_derivatives():
    """J and H of ndt_ref.point_terms (products of differentiated elementary rotations) against mpmath's numerical
    differentiation of a -> R(a) x, and the chain rule of pair_sums against the differentiated score of one pair."""
    ang, x = [0.3, -0.2, 0.5], np.array([[0.7, -1.1, 0.4]], np.float32)
    y0, J, H = R.point_terms(x, [0, 0, 0] + ang, ang, pcl_d1=False)[0]
    xv = mp.matrix([mp.mpf(float(v)) for v in x[0]])
    f = lambda k: (lambda a, b, c: (R.rotation([a, b, c]) * xv)[k])
    for k in range(3):
        for a in range(3):
            o = [0, 0, 0]
            o[a] = 1
            assert abs(mp.diff(f(k), ang, tuple(o)) - J[3 + a][k]) < mp.mpf(10) ** -25
            for b in range(a, 3):
                o2 = list(o)
                o2[b] += 1
                assert abs(mp.diff(f(k), ang, tuple(o2)) - H[(3 + a, 3 + b)][k]) < mp.mpf(10) ** -20
    g = R.grid(PASS["all_pass"]["tgt"], 1.0)
    v, (d1, d2) = g["vox"][0], R.gauss_constants(1.0)
    base = mp.matrix([mp.mpf("0.1"), mp.mpf("-0.05"), mp.mpf("0.02")])

    def score(*p):
        z = R.rotation(list(p[3:6])) * xv + mp.matrix(list(p[0:3])) - R.rotation(ang) * xv + base      # (= base at p0)
        return -d1 * mp.exp(-d2 / 2 * (z.T * v["icov"] * z)[0])
    p0 = [0, 0, 0] + ang
    t, _, _ = R.pair_sums(base + v["mean"], J, H, v, d1, d2)
    assert abs(score(*p0) - t[0]) < mp.mpf(10) ** -40
    for a in range(6):
        o = [0] * 6
        o[a] = 1
        assert abs(mp.diff(score, p0, tuple(o)) - t[1 + a]) < mp.mpf(10) ** -20
    for k, (a, b) in enumerate(R._PAIRS):
        o = [0] * 6
        o[a] += 1
        o[b] += 1
        assert abs(mp.diff(score, p0, tuple(o)) - t[7 + k]) < mp.mpf(10) ** -15, (a, b)


def test_pcl_d1_is_the_only_departure_from_the_derivative(orc, grids):
    """The engine's contract is PCL's Hessian; PCL's differs from the derivative in H[4][4] alone, by the one term of
    h_ang_d1 -- and not at all under the snap."""
    c = PASS["all_pass"]
    g = grids(c)
    pcl = R.derivatives(c["src"], g, 1.0, c["pose"], xprime="f32")
    true = R.derivatives(c["src"], g, 1.0, c["pose"], xprime="f32", pcl_d1=False)
    diff = np.abs(pcl["sums"] - true["sums"]) / pcl["scale"]
    k44 = 7 + R._PAIRS.index((4, 4))
    assert diff[k44] > 1e-4 and np.delete(diff, k44).max() == 0.0
    _, got = _against_oracle(_oracle(orc, c["tgt"], 1.0, 1), g, c["src"], 1.0, c["pose"], orc.NdtParams.reference())
    assert abs(got[k44] - pcl["sums"][k44]) <= R.DERIV_BAR * pcl["scale"][k44] < abs(got[k44] - true["sums"][k44])
    s = PASS["v63_n3_snap_a"]
    a = R.derivatives(s["src"], grids(s), 1.0, [0, 0, 0, 0.5e-4, 0.5e-4, 0.5e-4], xprime="f32")
    b = R.derivatives(s["src"], grids(s), 1.0, [0, 0, 0, 0.5e-4, 0.5e-4, 0.5e-4], xprime="f32", pcl_d1=False)
    np.testing.assert_array_equal(a["sums"], b["sums"])
