"""The NDT kernel set on the paths tests/test_ndt_gpu.py does not reach, against tests/ndt_ref.py (a slow NDT from the
definition: exact moments, 60-digit derivatives), which tests/test_ndt_ref_cpu.py has shown right first.  Bounds: means,
covariances and inverses within ndt_ref.grid_bounds (derived from the exact moments); score / gradient / Hessian within
ndt_ref.DERIV_BAR of each sum's scale against the reference at x' EXACT (the bar is 4 x the reference's own float32 gap),
and, far sharper, within ndt_ref.F64_BAR of its fscale (f64 rounding alone, about 1e-11 of scale) against the reference at
x' in FLOAT32 on the kernel's own table, which check_grid judges in the same test; plus gamma_pairs of the scale for the
large tiled sources.  No tolerance here was tuned to the kernel's output.

case (tests/ndt_cases.py)      branch it reaches
-----------------------------  ------------------------------------------------------------------------------------------
keys32_div1290                 n_leaves = 1290^3 < 2^31 - 1: 32-bit keys, key_bits = 31, the invalid key one above every leaf's
keys64_div1291                 n_leaves = 1291^3 >= 2^31 - 1: k_ndt_keys<unsigned long long>, the 64-bit radix plan
keys64_far                     80001^3 leaves (47 key bits), every div still an int
few_leaves_fewer_points        few_leaves (216 leaves <= 256) with nseg_launch = nfin = 26 < n_leaves, a box mostly empty;
                               PCL-centroid mode switches few_leaves off at a size where it would be on
occupied_2048 / occupied_2049  n_parts 16 / 1 (2048 / 2049 OCCUPIED leaves, 230 kept); voxels of 6..15 points over 16 parts;
                               dropped leaves of 1..5 points between kept ones; runs of 256 / 257 at n_parts = 1
runs_on_the_block_stride       runs of 255 / 256 / 257 and 4095 / 4096 / 4097 = 16 x 256 +- 1 (the stride of k_ndt_voxel_stats)
min_points_interleaved         counts 1..8: 5 dropped, 6 and 7 kept; dropped leaves shift table, counts and csum[v]
binning_edges                  x exactly on float32(k * 0.3), negative coordinates, -0.0, NaN / +-inf in one coordinate only
no_finite_point                a target without a finite point (nfin == 0)
voxel_far_from_origin          the single-pass covariance 4 x 10^3 m from the origin, spread 0.2 m
flat_exact / collinear_exact / coincident (degenerate), isotropic
                               the eigenvalue floor where l_min is 0 up to rounding; l_max = 0: the inverse zeroed
v1_n1 .. v129_n513             n in {1, 3, 511, 512, 513} (n < 512: empty workgroups, per_block = 1), n_vox in {1, 63, 64, 65,
                               128, 129} (chunks of exactly 64 and ragged); snap_a / snap_b: angles under, on, over 10e-5
all_pass / none_pass           every pair passes / none does;   empty_source: n = 0
staged_nonfinite               non-finite records (w = 0) in a source staged in LDS, one record per workgroup; the aligned cloud
zero_inverse                   a voxel with a zeroed inverse: e = 1, d2 e < 1, score only
(no case)                      the rejection `e > 1 || e < 0 || e != e` firing: d2 < 1 at every resolution and e <= 1, so on a
                               finite table it cannot fire; it is the one listed branch that no case reaches
large_262144                   512 points per workgroup: staged in LDS (<= kSrcCap); every lane of a trip passes: held >= 64
large_262145 / large_1000003   513 / 1954 per workgroup: the unstaged read src[lo + pi]
(all large)                    non-finite records (w = 0) on wave edges and on the pass's workgroup edges for that n
                               (ndt_cases.bad_at: per_block - 1, per_block, per_block + 1, ...); the aligned cloud keeps them
"""
import numpy as np
import pytest

import ndt_cases as K
import ndt_ref as R

pytestmark = pytest.mark.gpu
GRID = {c["name"]: c for c in K.grid_cases()}
PASS = {c["name"]: c for c in K.pass_cases()}


@pytest.fixture(scope="module")
def api(rs):
    from rsreg_amd import api as a, lib
    lib.build()
    if a.device_count() < 1:
        pytest.fail("no HIP device: the product has no CPU fallback")
    return a


@pytest.fixture(scope="module")
def refs():
    """Reference grids and derivatives, computed once and shared."""
    memo = {}

    def grid(c):
        if ("g", c["name"]) not in memo:
            memo["g", c["name"]] = R.grid(c["tgt"], c["res"])
        return memo["g", c["name"]]

    def deriv(c):
        if ("d", c["name"]) not in memo:
            memo["d", c["name"]] = R.derivatives(c["src"], grid(c), c["res"], c["pose"])
        return memo["d", c["name"]]

    def deriv_on(c, m):
        """at x' in float32, on the table `m` of the implementation"""
        return R.derivatives(c["src"], R.with_table(grid(c), m), c["res"], c["pose"], xprime="f32")
    grid.deriv, grid.deriv_on = deriv, deriv_on
    return grid


def _ndt(api, rs, src, tgt, res, pcl=False, ctx=None, device=False):
    n = api.NormalDistributionsTransform(ctx or api.default_context())
    n.params = api.ndt_params(reference=True, resolution=res)
    n.setPclCentroids(pcl)
    cloud = rs.PointCloud.from_xyz(tgt, is_dense=False)
    n.setInputSource(rs.PointCloud.from_xyz(src, is_dense=False))
    n.setInputTarget(api.DeviceCloud(cloud, ctx=n.ctx) if device else cloud)
    return n


def _oracle_table(orc, c):
    o = orc.NdtOracle()
    o.set_centroid_mode(1)
    o.set_target(np.ascontiguousarray(np.c_[c["tgt"], np.ones(len(c["tgt"]), np.float32)]), c["res"])
    return o.voxels()[0]


@pytest.mark.parametrize("device", [False, True], ids=["host", "devicecloud"])
@pytest.mark.parametrize("pcl", [False, True], ids=["mean", "pclsum"])
@pytest.mark.parametrize("name", list(GRID))
def test_grid_case(api, rs, orc, refs, name, pcl, device):
    c = GRID[name]
    g = refs(c)
    e = c["expect"]
    for k in ("div", "n_leaves", "occupied", "n_finite"):     # the value that selects the branch, from the reference
        if k in e:
            assert g[k] == e[k]
    src = c["tgt"][np.isfinite(c["tgt"]).all(1)][:64] if g["n_finite"] else np.zeros((4, 3), np.float32)
    n = _ndt(api, rs, src, c["tgt"], c["res"], pcl=pcl, device=device)
    m, cnt = n.voxels()
    assert len(cnt) == len(g["vox"])
    R.check_grid(c, g, m, cnt, n.centroids(), pcl_mode=pcl, oracle_m=_oracle_table(orc, c) if c["degenerate"] else None)
    n.align()
    assert n.result.n_voxels == len(g["vox"])


def _within(got, want, bound, what):
    err = np.abs(got - want)
    print("%s: worst err / bound: %.3g" % (what, float(np.max(err / np.maximum(bound, 1e-300)))))
    assert (err <= bound).all(), (what, err / np.maximum(bound, 1e-300))


@pytest.mark.parametrize("name", list(PASS))
def test_pass_case(api, rs, refs, name):
    c = PASS[name]
    g, d = refs(c), refs.deriv(c)
    assert (len(c["src"]), len(g["vox"])) == (c["expect"]["n"], c["expect"]["n_vox"])
    if "pairs" in c["expect"]:
        assert d["pairs"] == c["expect"]["pairs"]
    n = _ndt(api, rs, c["src"], c["tgt"], c["res"])
    m, cnt = n.voxels()
    assert len(cnt) == c["expect"]["n_vox"]
    R.check_grid({"name": name, "degenerate": name == "zero_inverse"}, g, m, cnt, n.centroids(), pcl_mode=False)
    got = R.pack(*n.derivatives(np.asarray(c["pose"], np.float64)))
    _within(got, d["sums"], R.DERIV_BAR * d["scale"], "x' exact")
    f = refs.deriv_on(c, m)
    np.testing.assert_array_equal(f["inc"], d["inc"])
    _within(got, f["sums"], R.F64_BAR * f["fscale"], "x' float32, own table")
    if "bad" in c:
        out = n.align()
        _check_aligned(n, out.xyz, out.points["w"], c["src"], c["bad"])


@pytest.fixture(scope="module")
def large(api, rs, refs):
    c = PASS["all_pass"]
    m = _ndt(api, rs, c["src"], c["tgt"], c["res"]).voxels()[0]     # (the table is the target's alone; test_pass_case judges it)
    return c, refs(c), refs.deriv(c), refs.deriv_on(c, m)


def _check_aligned(n, out_xyz, out_w, src, bad):
    T = n.getFinalTransformation()
    fin = np.ones(len(src), bool)
    fin[bad] = False
    want = R.transform_f32(T[:3, :], src[fin])
    np.testing.assert_array_equal(out_xyz[fin].view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(out_xyz[bad].view(np.uint32), src[bad].view(np.uint32))     # non-finite records: unchanged
    assert (out_w == 1.0).all()


@pytest.mark.parametrize("n_src", K.LARGE_N)
def test_large_tiled_source(api, rs, large, n_src):
    """A million-point source without a million mpmath evaluations: the 96 points of `all_pass` repeated in shuffled order
    (the sums are additive over points: the reference is sum_i mult_i row_i), non-finite records on wave and workgroup edges."""
    c, g, d, f = large
    src, mult, bad = K.tiled_source(c["src"], n_src, seed=n_src)
    per_block = -(-n_src // K.PASS_BLOCKS)
    assert (per_block <= 512) == (n_src == 262144) and len(src) == n_src and mult.sum() == n_src - len(bad)
    assert {per_block - 1, per_block, per_block + 1, n_src - 1} <= set(bad) and 0 not in bad and mult.min() > 0
    n = _ndt(api, rs, src, c["tgt"], c["res"])
    pairs = int(mult.sum()) * 8
    gamma = pairs * R.U / (1 - pairs * R.U)
    got = R.pack(*n.derivatives(np.asarray(c["pose"], np.float64)))
    want, scale, _ = R.total(d, mult)
    _within(got, want, (R.DERIV_BAR + gamma) * scale, "x' exact")
    want, scale, fscale = R.total(f, mult)
    _within(got, want, R.F64_BAR * fscale + gamma * scale, "x' float32, own table")
    out = n.align()
    _check_aligned(n, out.xyz, out.points["w"], src, bad)
    nd = _ndt(api, rs, src, c["tgt"], c["res"])
    nd.setInputSource(api.DeviceCloud(rs.PointCloud.from_xyz(src, is_dense=False), ctx=nd.ctx))
    dl = nd.align().download()
    assert bytes(nd.result.transform) == bytes(n.result.transform)
    _check_aligned(nd, dl.xyz, dl.points["w"], src, bad)


@pytest.mark.parametrize("name", ["v64_n511_general", "large"])
def test_line_search_repeats_bit_for_bit_in_a_fresh_context(api, rs, name):
    c = PASS["all_pass"] if name == "large" else PASS[name]
    src = K.tiled_source(c["src"], 262145, seed=3)[0] if name == "large" else c["src"]
    guess = np.eye(4, dtype=np.float32)
    guess[:3, 3] = (0.02, -0.01, 0.015)

    def run():
        n = _ndt(api, rs, src, c["tgt"], c["res"], ctx=api.Context(0))
        out = n.align(guess)
        r = n.result
        return bytes(r.transform), r.score, r.iterations, r.n_derivative_passes, r.converged, out.xyz.tobytes()
    base = run()
    assert run() == base and base[3] > 1
