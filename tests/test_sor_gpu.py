"""pcl::PassThrough and pcl::StatisticalOutlierRemoval on the GPU (rsreg_cloud_passthrough, rsreg_cloud_sor,
rsreg_cloud_knn_mean_distance, the Python and C++ adaptors) against tests/sor_ref.py.

The k-NN mean distances must be BIT-EQUAL to the reference for every record: both sides take the k + 1 smallest float32
squared distances, sort them, and add their float square roots in double in ascending order -- equal distances are equal
values, so no tie order enters.  mean / stddev / threshold agree to 1e-12 relative (f64 slabs in a fixed order against a
sequential sum; equal bits on the lattice, where every sum is exact).  The kept records equal the reference's wherever no
reference distance lies within 1e-9 relative of the reference threshold -- a condition on the INPUT that is asserted on
the reference alone.  Margins measured with the reference (mean_k = 50, 1.5 sigma; frame, form: closest distance to the
threshold, relative):
    render_frame(1, "50k")  raw 1.75e-05 (threshold 0.0596315,  895 removed)   after PassThrough 4.38e-06 (0.0549797, 1 726)
    render_frame(1, "N300") raw 6.78e-06 (threshold 0.0265525, 7 204 removed)  after PassThrough 1.74e-05 (0.0249845, 11 722)
    render_frame(0, "N300") raw 7.13e-06 (threshold 0.0266004, 7 136 removed)  after PassThrough 1.94e-05 (0.0250073, 11 840)
Thin, far, piled-up and cell-aligned clouds (the other rules of the grid's layout): tests/test_pointgrid_searches_gpu.py.
"""
import os
import subprocess

import numpy as np
import pytest

import sor_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 2.0 ** -6
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    return api


@pytest.fixture(scope="module")
def ctx(api):
    return api.Context(0)


def _cloud(xyz, width=None, height=1, is_dense=False, seed=0):
    """Records with a colour and a w of their own each, so that a record that moved or lost a byte shows."""
    from rsreg_amd import POINT_DTYPE, PointCloud
    rng = np.random.default_rng(seed)
    pts = np.zeros(len(xyz), POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["w"] = rng.random(len(xyz)).astype(np.float32)
    pts["rgba"] = rng.integers(0, 2 ** 32, len(xyz), dtype=np.uint32)
    raw = pts.view(np.uint8).reshape(len(xyz), 32)
    raw[:, 20:] = rng.integers(0, 256, (len(xyz), 12), dtype=np.uint8)   # (the padding travels too)
    return PointCloud(pts, width=len(xyz) if width is None else width, height=height, is_dense=is_dense)


def _bytes(points):
    return np.ascontiguousarray(points).view(np.uint8).reshape(len(points), -1)


def _same_records(got, src, mask=None):
    """All 32 bytes of every record, in order; mask: the records of `src` that are expected (taken through the byte view:
    numpy's own indexing of a padded structured array copies the fields only)."""
    want = _bytes(src) if mask is None else _bytes(src)[mask]
    return _bytes(got).shape == want.shape and bool((_bytes(got) == want).all())


def _frame(frame, size, passed=False):
    from rsreg_amd import PointCloud, synth
    fr = synth.render_frame(frame, size)
    if not passed:
        return fr
    pts = fr.points[S.passthrough_keep(fr.xyz, 2, 0.2, 2.5)]
    return PointCloud(np.ascontiguousarray(pts), width=len(pts), height=1, is_dense=True)


def lattice(m):
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)
    return (g * H + np.array([0.0, 0.0, 1.0])).astype(np.float32)


def _assert_bit_equal(api, ctx, cloud, k):
    got = api.DeviceCloud(cloud, ctx=ctx).knn_mean_distance(k)
    want = S.knn_mean_distance(cloud.xyz, k)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    print("knn_mean_distance: n = %d, mean_k = %d, records that differ: %d" % (len(cloud), k, len(bad)))
    assert len(bad) == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    return got


# ------------------------------------------------------------------------------------------------ k-NN mean distance
def test_knn_lattice_exact(api, ctx):
    xyz = lattice(12)
    got = _assert_bit_equal(api, ctx, _cloud(xyz), 6)
    g = np.rint((xyz - np.array([0, 0, 1], np.float32)) / H).astype(int)
    inner = ((g > 0) & (g < 11)).all(axis=1)
    assert (got[inner] == np.float32(H)).all()


@pytest.mark.parametrize("n,seed", [(1000, 1), (5000, 2), (20000, 3)])
@pytest.mark.parametrize("k", [1, 8, 50, 64])
def test_knn_random_clouds(api, ctx, n, seed, k):
    rng = np.random.default_rng(seed)
    xyz = (rng.random((n, 3)) * np.array([2.0, 1.5, 0.7]) + np.array([-1.0, -0.5, 0.4])).astype(np.float32)
    _assert_bit_equal(api, ctx, _cloud(xyz), k)


@pytest.mark.parametrize("size", ["50k", "N300", "N1M"])
@pytest.mark.parametrize("passed", [False, True], ids=["raw", "passthrough"])
def test_knn_rendered_frames(api, ctx, size, passed):
    _assert_bit_equal(api, ctx, _frame(1, size, passed), 50)


def test_knn_non_finite_records(api, ctx):
    rng = np.random.default_rng(4)
    xyz = rng.random((6000, 3)).astype(np.float32)
    xyz[rng.integers(0, 6000, 300)] = np.nan
    xyz[rng.integers(0, 6000, 300), 1] = np.inf
    xyz[rng.integers(0, 6000, 100), 2] = -np.inf
    got = _assert_bit_equal(api, ctx, _cloud(xyz), 20)
    assert (got[~S.finite_rows(xyz)] == 0).all()


def test_knn_every_point_three_times(api, ctx):
    rng = np.random.default_rng(5)
    xyz = np.repeat(rng.random((3000, 3)).astype(np.float32), 3, axis=0)[rng.permutation(9000)]
    assert (_assert_bit_equal(api, ctx, _cloud(xyz), 2) == 0).all()
    _assert_bit_equal(api, ctx, _cloud(xyz), 10)


def test_knn_cloud_in_one_plane(api, ctx):
    rng = np.random.default_rng(6)
    xyz = rng.random((8000, 3)).astype(np.float32)
    xyz[:, 2] = np.float32(1.25)
    _assert_bit_equal(api, ctx, _cloud(xyz), 30)
    xyz[:, 1] = np.float32(-0.5)                          # ... and on one line
    _assert_bit_equal(api, ctx, _cloud(xyz), 30)


@pytest.mark.parametrize("k", [1, 50, 64])
def test_knn_exactly_k_plus_one_points(api, ctx, k):
    rng = np.random.default_rng(7)
    _assert_bit_equal(api, ctx, _cloud(rng.random((k + 1, 3)).astype(np.float32)), k)


def test_knn_errors(api, ctx):
    from rsreg_amd import lib
    rng = np.random.default_rng(8)
    xyz = rng.random((40, 3)).astype(np.float32)
    dc = api.DeviceCloud(_cloud(xyz), ctx=ctx)
    for k in (0, 65, 40):                                  # below 1, above the cap, more than the cloud holds
        with pytest.raises(lib.RsregError) as e:
            dc.knn_mean_distance(k)
        assert e.value.status == lib.RSREG_ERR_INVALID_ARG
    xyz[:5] = np.nan
    dc = api.DeviceCloud(_cloud(xyz), ctx=ctx)
    dc.knn_mean_distance(34)
    with pytest.raises(lib.RsregError):
        dc.knn_mean_distance(35)                          # 35 finite records only
    one = np.array([[0, 0, 1], [np.nan, 0, 0]], np.float32)
    sor = api.StatisticalOutlierRemoval()
    sor.setInputCloud(api.DeviceCloud(_cloud(one), ctx=ctx))
    with pytest.raises(lib.RsregError) as e:
        sor.filter()
    assert e.value.status == lib.RSREG_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ StatisticalOutlierRemoval
def _sor(api, ctx, cloud, k, mult, negative=False):
    sor = api.StatisticalOutlierRemoval()
    sor.setInputCloud(cloud if isinstance(cloud, api.DeviceCloud) else api.DeviceCloud(cloud, ctx=ctx))
    sor.setMeanK(k)
    sor.setStddevMulThresh(mult)
    sor.setNegative(negative)
    out = sor.filter()
    return out, sor.stats


def _check_sor(api, ctx, cloud, k, mult, negative=False, exact_stats=False):
    out, st = _sor(api, ctx, cloud, k, mult, negative)
    got = out.download()
    keep, dist, (n_valid, mean, stddev, thr) = S.sor(cloud.xyz, k, mult, negative)
    print("sor: n = %d, n_valid = %d / %d, mean %r / %r, stddev %r / %r, threshold %r / %r, kept %d / %d" %
          (len(cloud), st.n_valid, n_valid, st.mean, mean, st.stddev, stddev, st.threshold, thr, st.n_kept, int(keep.sum())))
    assert st.n_valid == n_valid
    if exact_stats:
        assert (st.mean, st.stddev, st.threshold) == (mean, stddev, thr)
    else:
        for a, b in ((st.mean, mean), (st.stddev, stddev), (st.threshold, thr)):
            assert abs(a - b) <= 1e-12 * abs(b)
    # byte for byte and in order, with the engine's own threshold
    own = S.sor_keep(cloud.xyz, dist, st.threshold, negative)
    assert st.n_kept == len(got) == int(own.sum())
    assert _same_records(got.points, cloud.points, own)
    assert (got.width, got.height, got.is_dense) == (len(got), 1, cloud.is_dense)
    # the reference's kept set: the input keeps every distance clear of the threshold (asserted on the reference alone)
    margin = S.threshold_margin(dist, cloud.xyz, thr) if thr != 0 else np.inf
    print("     closest reference distance to the reference threshold: %.3g relative" % margin)
    assert margin > 1e-9
    assert _same_records(got.points, cloud.points, keep)
    return got, st


def test_sor_lattice_equal_bits(api, ctx):
    """mean_k = 1 on the lattice with two outliers 32 H and 64 H beyond a corner, along an axis: every distance is H, 32 H or
    64 H, so every sum and square is exact in double whatever the order -- the statistics must have equal bits."""
    xyz = lattice(10)
    xyz = np.concatenate([xyz, np.array([[0, 0, 1.0 + (9 + 32) * H], [(9 + 64) * H, 9 * H, 1.0 + 9 * H]], np.float32)])
    got, st = _check_sor(api, ctx, _cloud(xyz), 1, 1.0, exact_stats=True)
    assert st.mean == (1000 * H + 96 * H) / 1002 and len(got) == 1000
    _check_sor(api, ctx, _cloud(xyz), 6, 1.0)              # (irrational distances at the faces: 1e-12)


@pytest.mark.parametrize("frame,size", [(1, "50k"), (1, "N300"), (0, "N300")])
@pytest.mark.parametrize("passed", [False, True], ids=["raw", "passthrough"])
def test_sor_rendered_frames(api, ctx, frame, size, passed):
    got, st = _check_sor(api, ctx, _frame(frame, size, passed), 50, 1.5)
    if (frame, size, passed) == (1, "N300", False):
        assert len(_frame(frame, size)) - len(got) == 7204 and abs(st.threshold - 0.02655) < 1e-5


def test_sor_non_finite_kept_and_negative(api, ctx):
    rng = np.random.default_rng(9)
    xyz = (rng.standard_normal((7000, 3)) * 0.3).astype(np.float32)
    xyz[rng.integers(0, 7000, 200)] = np.nan
    xyz[rng.integers(0, 7000, 200), 0] = np.inf
    cloud = _cloud(xyz, seed=3)
    got, _ = _check_sor(api, ctx, cloud, 16, 1.0)
    assert (~S.finite_rows(got.xyz)).sum() == (~S.finite_rows(xyz)).sum()      # PCL's quirk: all of them stay
    neg, _ = _check_sor(api, ctx, cloud, 16, 1.0, negative=True)
    assert S.finite_rows(neg.xyz).all() and len(neg) + len(got) == len(cloud)


def test_sor_defaults_are_pcl_s(api, ctx):
    rng = np.random.default_rng(10)
    cloud = _cloud(rng.random((3000, 3)).astype(np.float32))
    sor = api.StatisticalOutlierRemoval()
    sor.setInputCloud(cloud)                               # a host cloud: through a temporary DeviceCloud
    out = sor.filter()
    keep, _, _ = S.sor(cloud.xyz, 1, 0.0)
    assert _same_records(out.points, cloud.points, keep)


# ------------------------------------------------------------------------------------------------ PassThrough
def _pass(api, cloud, field, lo=None, hi=None, negative=False, keep_organized=False):
    p = api.PassThrough()
    p.setInputCloud(cloud)
    p.setFilterFieldName(field)
    if lo is not None:
        p.setFilterLimits(lo, hi)
    p.setNegative(negative)
    p.setKeepOrganized(keep_organized)
    return p.filter()


@pytest.mark.parametrize("field", ["x", "y", "z"])
@pytest.mark.parametrize("negative", [False, True])
def test_passthrough_bytes(api, ctx, field, negative):
    rng = np.random.default_rng(20)
    xyz = np.round(rng.standard_normal((30000, 3)) * 64).astype(np.float32) / 64   # many records exactly on a limit
    xyz[rng.integers(0, 30000, 500)] = np.nan
    xyz[rng.integers(0, 30000, 500), 2] = np.inf
    cloud = _cloud(xyz, width=300, height=100, seed=4)
    f = "xyz".index(field)
    lo, hi = np.float32(-0.5), np.float32(0.75)
    assert (xyz[:, f] == lo).any() and (xyz[:, f] == hi).any()
    dc = api.DeviceCloud(cloud, ctx=ctx)
    out = _pass(api, dc, field, lo, hi, negative).download()
    want, _ = S.passthrough(cloud.points, f, lo, hi, negative)
    assert _same_records(out.points, want)
    assert (out.width, out.height, out.is_dense) == (len(want), 1, True)
    org = _pass(api, dc, field, lo, hi, negative, keep_organized=True).download()
    want_org, _ = S.passthrough(cloud.points, f, lo, hi, negative, keep_organized=True)
    assert _same_records(org.points, want_org)
    assert (org.width, org.height, org.is_dense) == (300, 100, False)
    removed = np.isnan(org.points["x"]) & ~np.isnan(cloud.points["x"])
    assert (org.points["x"][removed].view(np.uint32) == 0x7fc00000).all()       # the quiet NaN


def test_passthrough_defaults_empty_result_and_metadata(api, ctx):
    from rsreg_amd import lib
    fr = _frame(1, "50k")
    dc = api.DeviceCloud(fr, ctx=ctx)
    out = _pass(api, dc, "z").download()                   # FLT_MIN .. FLT_MAX: the records at the origin go
    want, _ = S.passthrough(fr.points, 2)
    assert _same_records(out.points, want) and 0 < len(out) < len(fr)
    empty = _pass(api, dc, "z", 100.0, 200.0).download()
    assert (len(empty), empty.width, empty.height, empty.is_dense) == (0, 0, 1, True)
    # keep_organized with nothing removed: is_dense stays the input's
    dense = _cloud(np.random.default_rng(21).random((600, 3)).astype(np.float32), width=30, height=20, is_dense=True)
    same = _pass(api, api.DeviceCloud(dense, ctx=ctx), "x", -1.0, 2.0, keep_organized=True).download()
    assert _same_records(same.points, dense.points) and (same.width, same.height, same.is_dense) == (30, 20, True)
    host = _pass(api, fr, "z", 0.2, 2.5)                   # a host cloud: through a temporary DeviceCloud
    assert _same_records(host.points, S.passthrough(fr.points, 2, 0.2, 2.5)[0])
    with pytest.raises(lib.RsregError) as e:
        _pass(api, dc, "rgb")
    assert e.value.status == lib.RSREG_ERR_INVALID_ARG
    assert ctx.h and lib.lib().rsreg_cloud_passthrough(ctx.h, dc.h, 3, 0.0, 1.0, 0, 0, dc.h) == lib.RSREG_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ both filters
def test_in_place_versions_and_repeatability(api, ctx):
    import ctypes as C

    from rsreg_amd import lib
    fr = _frame(1, "50k")
    L = lib.lib()
    want_pass = S.passthrough(fr.points, 2, 0.2, 2.5)[0]
    runs = []
    for _ in range(2):
        dc = api.DeviceCloud(fr, ctx=ctx)
        v0 = dc.stamp
        lib.check(L.rsreg_cloud_passthrough(ctx.h, dc.h, 2, 0.2, 2.5, 0, 0, dc.h), ctx.h)     # in == out
        v1 = dc.stamp
        assert v1[0] == v0[0] and v1[1] != v0[1]
        after_pass = dc.download()
        assert _same_records(after_pass.points, want_pass)
        st = lib.SorStats()
        lib.check(L.rsreg_cloud_sor(ctx.h, dc.h, 50, 1.5, 0, dc.h, C.byref(st)), ctx.h)        # in == out
        assert dc.stamp[1] != v1[1]
        lib.check(L.rsreg_cloud_sor(ctx.h, dc.h, 50, 1.5, 0, dc.h, None), ctx.h)               # stats may be NULL
        runs.append((after_pass.points.tobytes(), st.threshold, st.n_kept))
    assert runs[0] == runs[1]
    # out of place gives the same bytes as in place
    dc = api.DeviceCloud(fr, ctx=ctx)
    p = _pass(api, dc, "z", 0.2, 2.5)
    out, st = _sor(api, ctx, p, 50, 1.5)
    assert (st.threshold, st.n_kept) == runs[0][1:]
    keep, _, _ = S.sor(np.stack([want_pass["x"], want_pass["y"], want_pass["z"]], 1), 50, 1.5)
    assert _same_records(out.download().points, want_pass, keep)


def test_filters_leave_an_alignment_alone(api, ctx):
    """Between set_target and align of an ICP on the same context: the alignment's result and getFitnessScore do not move."""
    from rsreg_amd import synth
    tgt, src = synth.render_frame(0, "50k", "parity"), synth.render_frame(1, "50k", "parity")

    def run(disturb):
        c = api.Context(0)
        icp = api.IterativeClosestPoint(c)
        icp.params = api.icp_params(reference=True)
        icp.setInputSource(src)
        icp.setInputTarget(tgt)
        if disturb:
            dc = api.DeviceCloud(src, ctx=c)
            _sor(api, c, _pass(api, dc, "z", 0.2, 2.5), 50, 1.5)
            dc.knn_mean_distance(8)
        icp.align()
        score = icp.getFitnessScore()
        if disturb:
            _sor(api, c, api.DeviceCloud(tgt, ctx=c), 20, 1.0)
            assert icp.getFitnessScore() == score
        return icp.getFinalTransformation().tobytes(), icp.result.iterations, icp.result.n_correspondences, score

    assert run(False) == run(True)


def test_cpp_adaptor_prefilter(api, ctx, tmp_path):
    """tests/cpp/sor_runner.cpp: the reference's pre-filter sequence against rsreg::, host clouds and device clouds."""
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "sor_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sor_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    fr = _frame(1, "50k")
    fr.points.tofile(str(tmp_path / "in.bin"))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(fr.width), str(fr.height), str(tmp_path / "host.bin"), str(tmp_path / "dev.bin")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    vals = dict(l.split() for l in r.stdout.strip().splitlines())
    p = _pass(api, api.DeviceCloud(fr, ctx=ctx), "z", 0.2, 2.5)
    want, st = _sor(api, ctx, p, 50, 1.5)
    want = want.download().points
    for name in ("host.bin", "dev.bin"):
        got = np.fromfile(str(tmp_path / name), dtype=fr.points.dtype)
        assert _same_records(got, want)
    assert int(vals["kept"]) == int(vals["kept_device"]) == len(want) == int(vals["width"]) and vals["height"] == "1"
    assert float.fromhex(vals["threshold"]) == st.threshold
