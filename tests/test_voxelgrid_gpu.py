"""GPU: pcl::VoxelGrid on the device (csrc/voxel.hip: rsreg_cloud_voxel_grid, rsreg_voxel_grid_gpu) against the host restatement
(rsreg_voxel_grid) and the numpy reference (tests/voxelgrid_ref.py): record bytes and the info struct, equal.  The clouds are
those of tests/voxelgrid_cases.py -- every run-length class of the sum kernels, leaf boundaries and signs, every key width, the
minimum number of points, both centroid modes, the edge inputs -- the CPU tests show what each of them covers."""
import numpy as np
import pytest

import voxelgrid_cases as V
import voxelgrid_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(rs):
    from rsreg_amd import api, lib as L
    L.build()
    if api.device_count() < 1:
        pytest.fail("no HIP device: the product has no CPU fallback")
    return L


@pytest.fixture(scope="module")
def ctx(lib):
    from rsreg_amd import api
    return api.Context(0)


def same_bytes(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("name", sorted(V.cases()))
def test_device_cloud_equals_host_and_reference(lib, ctx, name):
    pts, leaf, all_data, mp = V.cases()[name]
    want, want_info = V.reference(name)
    host, host_info = V.run_host(lib, pts, leaf, all_data, mp)
    dense = 0 if name == "overflow_1291" else 1      # (a cloud flagged dense although it holds non-finite records, as a rule)
    got, info, meta, (before, after) = V.run_gpu_cloud(lib, ctx, pts, leaf, all_data, mp, is_dense=dense)
    assert info == want_info == host_info
    same_bytes(got, want)
    same_bytes(got, host)
    if want_info["overflowed"]:
        assert meta == (len(pts), 32, len(pts), 1, dense)
    else:
        assert meta == (len(want), 32, len(want), 1, 1)
    assert after > before


@pytest.mark.parametrize("name", ["run_classes_min2", "non_finite_in_dense_cloud", "keys_32_bits_and_sentinel", "overflow_1291", "alpha_70000",
                                  "empty", "all_non_finite"])
def test_host_records_entry_point(lib, ctx, name):
    pts, leaf, all_data, mp = V.cases()[name]
    want, want_info = V.reference(name)
    got, info = V.run_gpu_host_records(lib, ctx, pts, leaf, all_data, mp)
    assert info == want_info
    same_bytes(got, want)


def wide_records(pts):
    wide = np.zeros(len(pts), V.POINT48)
    for f in ("x", "y", "z", "w", "rgba"):
        wide[f] = pts[f]
    wide["extra"] = 0xdeadbeef
    return wide


@pytest.mark.parametrize("name", ["run_classes_min0", "non_finite_in_dense_cloud"])
def test_stride_48(lib, ctx, name):
    """48-byte records: the payload behind the colour is not carried over, the output record is zero there"""
    pts, leaf, all_data, mp = V.cases()[name]
    want, want_info = V.reference(name)
    wide = wide_records(pts)
    got, info, meta, _ = V.run_gpu_cloud(lib, ctx, wide, leaf, all_data, mp)
    assert info == want_info and meta == (len(want), 48, len(want), 1, 1)
    for f in ("x", "y", "z", "w", "rgba"):
        np.testing.assert_array_equal(got[f].view(np.uint32), want[f].view(np.uint32))
    assert (got["extra"] == 0).all()
    host, _ = V.run_host(lib, wide, leaf, all_data, mp)
    same_bytes(got, host)


def test_stride_20_unaligned_records(lib, ctx):
    """the smallest record the filter takes (xyz, a float, the colour): no 16-byte loads possible"""
    pts, leaf, all_data, mp = V.cases()["run_classes_min0"]
    want, want_info = V.reference("run_classes_min0")
    dt = np.dtype({"names": ["x", "y", "z", "w", "rgba"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u4"], "offsets": [0, 4, 8, 12, 16], "itemsize": 20})
    small = np.zeros(len(pts), dt)
    for f in dt.names:
        small[f] = pts[f]
    got, info, meta, _ = V.run_gpu_cloud(lib, ctx, small, leaf, all_data, mp)
    assert info == want_info and meta == (len(want), 20, len(want), 1, 1)
    for f in dt.names:
        np.testing.assert_array_equal(got[f].view(np.uint32), want[f].view(np.uint32))


def test_in_place_bumps_the_version(lib, ctx):
    pts, leaf, all_data, mp = V.cases()["boundaries_l003"]
    want, want_info = V.reference("boundaries_l003")
    got, info, meta, (before, after) = V.run_gpu_cloud(lib, ctx, pts, leaf, all_data, mp, in_place=True, width=len(pts) // 2, height=2, is_dense=0)
    assert info == want_info and meta == (len(want), 32, len(want), 1, 1)
    same_bytes(got, want)
    assert after == before + 1
    # a leaf too small, in place: the cloud stays as it is, organized as it was
    pts2, leaf2, _, _ = V.cases()["overflow_1291"]
    got2, info2, meta2, (b2, a2) = V.run_gpu_cloud(lib, ctx, pts2, leaf2, 1, 0, in_place=True, width=5, height=2, is_dense=0)
    assert info2["overflowed"] == 1 and meta2 == (10, 32, 5, 2, 0) and a2 == b2
    same_bytes(got2, pts2)
    # ... and into another cloud: a copy with the input's shape
    got3, info3, meta3, (b3, a3) = V.run_gpu_cloud(lib, ctx, pts2, leaf2, 1, 0, width=5, height=2, is_dense=0)
    assert info3["overflowed"] == 1 and meta3 == (10, 32, 5, 2, 0) and a3 > b3
    same_bytes(got3, pts2)


def test_second_context_and_repeat_give_the_same_bytes(lib, ctx):
    from rsreg_amd import api
    other = api.Context(0)
    for name in ("run_classes_min0", "alpha_70000"):
        pts, leaf, all_data, mp = V.cases()[name]
        want, _ = V.reference(name)
        # the second context has run another filter on another cloud first: its scratch is used
        V.run_gpu_cloud(lib, other, V.cases()["boundaries_aniso"][0], (0.01, 0.02, 0.05), 1, 0)
        for c in (ctx, other, ctx):
            got, _, _, _ = V.run_gpu_cloud(lib, c, pts, leaf, all_data, mp)
            same_bytes(got, want)
    other.close()


@pytest.mark.parametrize("leaf", [0.01, 1.0])
def test_synthetic_frame_equals_host(rs, lib, ctx, leaf):
    """a rendered 640 x 480 frame: the real distribution of run lengths (0.01: ~10^5 leaves of a few points; 1.0: a handful of
    leaves of 10^4 .. 10^5 points, and at either leaf the pile of missing-depth records at the origin), with non-finite
    records scattered through it"""
    frame = rs.synth.render_frame(0, "N300", "parity")
    pts = R.raw_copy(frame.points)
    pts["z"][::997] = np.nan
    pts["x"][5::1999] = np.inf
    assert (pts["z"] == 0).sum() > 1024
    lf = (leaf, leaf, leaf)
    host, host_info = V.run_host(lib, pts, lf, 1, 0)
    got, info, meta, _ = V.run_gpu_cloud(lib, ctx, pts, lf, 1, 0, width=frame.width, height=frame.height, is_dense=0)
    assert info == host_info and meta == (len(host), 32, len(host), 1, 1)
    same_bytes(got, host)
    assert info["n_leaves"] == len(host) > (10000 if leaf == 0.01 else 1)


def test_python_layer(rs, lib, ctx):
    from rsreg_amd import api
    pts, leaf, _, _ = V.cases()["run_classes_min48"]
    want, want_info = V.reference("run_classes_min48")
    cloud = rs.PointCloud(R.raw_copy(pts), is_dense=False)
    dev = api.DeviceCloud(cloud, ctx=ctx)
    out = dev.voxel_grid(leaf, min_points=48)
    assert out.info() == (len(want), 32, len(want), 1, True)
    same_bytes(out.download().points, want)
    f = api.VoxelGrid(ctx)                              # a host cloud through the context: rsreg_voxel_grid_gpu
    f.setLeafSize(*leaf)
    f.setMinimumPointsNumberPerVoxel(48)
    f.setInputCloud(cloud)
    res = f.filter()
    same_bytes(res.points, want)
    assert (res.width, res.height, res.is_dense) == (len(want), 1, True)
    assert f.getNrDivisions().tolist() == want_info["div_b"] and f.getMinBoxCoordinates().tolist() == want_info["min_b"]
    g = api.VoxelGrid()
    g.setLeafSize(*leaf)
    g.setDownsampleAllData(False)
    g.setInputCloud(dev)
    xyz_only = g.filter()
    same_bytes(xyz_only.download().points, V.reference("run_classes_xyz_only")[0])
    assert g.info.n_leaves == len(V.RUN_LENGTHS)


def test_refused_arguments(lib, ctx):
    import ctypes as C
    pts = V.cases()["one_point"][0]
    h = V.Handle(lib, ctx, pts)
    out = V.Handle(lib, ctx)
    for leaf in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, np.inf), (np.nan, 1.0, 1.0)):
        p = V.params(lib, leaf, 1, 0)
        assert lib.lib().rsreg_cloud_voxel_grid(ctx.h, h.h, C.byref(p), out.h, None) == lib.RSREG_ERR_INVALID_ARG
    assert lib.lib().rsreg_cloud_voxel_grid(ctx.h, h.h, None, out.h, None) == lib.RSREG_ERR_INVALID_ARG
    p = V.params(lib, (1.0, 1.0, 1.0), 1, 0)
    assert lib.lib().rsreg_cloud_voxel_grid(ctx.h, h.h, C.byref(p), out.h, None) == 0 and out.info()[0] == 1
    h.close()
    out.close()
