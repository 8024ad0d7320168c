"""CPU: the host restatement of pcl::VoxelGrid (rsreg_voxel_grid, csrc/voxel_host.cpp) against the numpy reference written
from the contract (tests/voxelgrid_ref.py): record bytes and the info struct, equal.  And the reference against itself: its
cumulative sums are the sequential float sum, and the clouds of tests/voxelgrid_cases.py tell the order inside a leaf apart."""
import ctypes as C

import numpy as np
import pytest

import voxelgrid_cases as V
import voxelgrid_ref as R


@pytest.fixture(scope="module")
def lib(rs):
    from rsreg_amd import lib as L
    L.build()
    return L


@pytest.mark.parametrize("name", sorted(V.cases()))
def test_host_restatement_equals_reference(lib, name):
    pts, leaf, all_data, mp = V.cases()[name]
    want, want_info = V.reference(name)
    got, info = V.run_host(lib, pts, leaf, all_data, mp)
    assert info == want_info
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))


def test_cases_cover_what_they_claim():
    info = {k: V.reference(k)[1] for k in V.cases()}
    prod = lambda v: int(np.prod(np.asarray(v, np.int64)))
    assert info["keys_31_bits"]["div_b"] == [1290] * 3 and prod(info["keys_31_bits"]["div_b"]) - 1 >= 2 ** 30
    assert info["keys_31_bits_and_sentinel"]["n_finite"] == len(V.cases()["keys_31_bits_and_sentinel"][0]) - 1
    assert info["keys_32_bits"]["div_b"] == [1291] * 3 and 2 ** 31 < prod(info["keys_32_bits"]["div_b"]) < 2 ** 32
    assert info["keys_32_bits"]["overflowed"] == 0 and info["keys_32_bits_and_sentinel"]["overflowed"] == 0
    for k in ("overflow_1291", "two_points_1000_apart_xyz"):
        pts = V.cases()[k][0]
        assert info[k]["overflowed"] == 1 and info[k]["n_out"] == len(pts)
        assert V.reference(k)[0].tobytes() == pts.tobytes()            # the output is the input, non-finite records included
    assert info["two_points_1000_apart_x"]["overflowed"] == 0 and info["two_points_1000_apart_x"]["div_b"][0] > 999000
    assert info["two_points_1000_apart_x"]["n_out"] == 2
    assert info["boundaries_aniso"]["min_b"][0] < 0 and info["boundaries_l003"]["min_b"][2] < 0
    assert info["run_classes_min0"]["n_out"] == len(V.RUN_LENGTHS) and info["run_classes_min5000"]["n_out"] == 0
    assert info["run_classes_min2"]["n_out"] == len(V.RUN_LENGTHS) - 1 and info["run_classes_min48"]["n_out"] == len(V.RUN_LENGTHS) - 3
    assert info["run_classes_min1"]["n_out"] == len(V.RUN_LENGTHS)
    for k in ("empty", "all_non_finite"):
        assert info[k]["n_out"] == 0 and info[k]["n_finite"] == 0 and len(V.reference(k)[0]) == 0
    nf = info["non_finite_in_dense_cloud"]
    assert 0 < nf["n_finite"] < len(V.cases()["non_finite_in_dense_cloud"][0])


def test_run_classes_tell_the_order_inside_a_leaf_apart():
    """Every leaf of 47 points and more must come out with other bytes when its points are added in descending input index:
    otherwise a filter that adds them in the wrong order (an unstable sort) would pass."""
    pts, leaf, _, _ = V.cases()["run_classes_min0"]
    want, info = V.reference("run_classes_min0")
    rev, _ = R.voxel_grid(pts, leaf, True, 0, reverse_leaves=True)
    assert len(want) == len(rev) == len(V.RUN_LENGTHS)
    # leaf l lies at x in [l, l + 1): the output is in that order
    assert (np.floor(want["x"]).astype(int) == np.arange(len(V.RUN_LENGTHS))).all()
    for l, cnt in enumerate(V.RUN_LENGTHS):
        same = want[l].tobytes() == rev[l].tobytes()
        assert same == (cnt <= 2), (l, cnt)
    # and the input really is interleaved: the first 200 records touch most leaves
    first = np.floor(pts["x"][:200]).astype(int)
    assert len(set(first.tolist())) >= 6 and (np.diff(first) != 0).sum() > 100


def test_alpha_case_passes_2_24_and_depends_on_the_order():
    pts, leaf, _, _ = V.cases()["alpha_70000"]
    big = pts[(pts["x"] < 1.0)]
    assert len(big) >= 70000 and ((big["rgba"] >> 24) == 255).all() and 255 * len(big) > 2 ** 24
    want, _ = V.reference("alpha_70000")
    a_sum = R.sequential_sum((big["rgba"] >> 24).astype(np.float32))
    assert float(a_sum) != 255.0 * len(big)                 # (the float sum has rounded on the way: an integer sum gives other bits)
    assert want[0]["rgba"] >> 24 == int(np.uint32(a_sum / np.float32(len(big))))
    other = want[1:]["rgba"] >> 24
    assert ((other > 0) & (other < 255)).any()               # averaged alphas that are not a default


def test_reference_sums_are_sequential():
    """np.cumsum is the sum the contract defines (a Python loop of float32 additions), np.sum is not"""
    rng = np.random.default_rng(4)
    v = (rng.random(5000) * 1000).astype(np.float32)
    loop = R.sequential_sum(v)
    assert np.cumsum(v, dtype=np.float32)[-1].tobytes() == loop.tobytes()
    assert np.sum(v, dtype=np.float32).tobytes() != loop.tobytes()


def test_by_hand():
    """four points, leaf 1: the leaves of x = -0.5 and x = 0.5 differ (floor, not truncation), min_b = -1"""
    pts = V.make(np.array([[0.5, 0.25, 0.0], [-0.5, 0.25, 0.0], [0.75, 0.75, 0.5], [-0.25, 0.5, 0.5]], np.float32),
                 np.array([0x10204080, 0x30609010, 0x20406081, 0x50a0b030], np.uint32))
    out, info = R.voxel_grid(pts, (1.0, 1.0, 1.0))
    assert info["min_b"] == [-1, 0, 0] and info["max_b"] == [0, 0, 0] and info["div_b"] == [2, 1, 1] and info["divb_mul"] == [1, 2, 2]
    assert len(out) == 2
    assert (out["x"] == np.float32([-0.375, 0.625])).all() and (out["y"] == np.float32([0.375, 0.5])).all()
    assert (out["z"] == np.float32([0.25, 0.25])).all() and (out["w"] == 1.0).all()
    # bytes a r g b: (0x30 + 0x50) / 2, ... truncated
    assert out["rgba"][0] == (0x40 << 24) | (0x80 << 16) | (0xa0 << 8) | 0x20
    assert out["rgba"][1] == (0x18 << 24) | (0x30 << 16) | (0x50 << 8) | 0x80      # 0x81 + 0x80 = 257 -> 128.5 -> 128
    xyz_only, _ = R.voxel_grid(pts, (1.0, 1.0, 1.0), downsample_all_data=False)
    assert (xyz_only["rgba"] == 0xff000000).all() and (xyz_only["x"] == out["x"]).all()


def test_host_in_place_and_stride_48(lib):
    pts, leaf, all_data, mp = V.cases()["boundaries_l003"]
    want, want_info = V.reference("boundaries_l003")
    got, info = V.run_host(lib, pts, leaf, all_data, mp, in_place=True)
    assert info == want_info and got.tobytes() == want.tobytes()
    wide = np.zeros(len(pts), V.POINT48)
    for f in ("x", "y", "z", "w", "rgba"):
        wide[f] = pts[f]
    wide["extra"] = 0xdeadbeef                                   # (the output record is zeroed behind the colour)
    got48, info48 = V.run_host(lib, wide, leaf, all_data, mp)
    assert info48 == want_info and len(got48) == len(want)
    for f in ("x", "y", "z", "w", "rgba"):
        np.testing.assert_array_equal(got48[f].view(np.uint32), want[f].view(np.uint32))
    assert (got48["extra"] == 0).all()


def test_refused_arguments(lib):
    pts = np.ascontiguousarray(V.cases()["one_point"][0])
    out, n_out = np.zeros_like(pts), C.c_size_t(0)
    for leaf in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, np.inf), (np.nan, 1.0, 1.0), (1e-45, 1.0, 1.0)):
        lf = np.asarray(leaf, np.float32)
        rc = lib.lib().rsreg_voxel_grid(pts.ctypes.data, 1, 32, lf.ctypes.data, 1, 0, out.ctypes.data, C.byref(n_out), None)
        assert rc == lib.RSREG_ERR_INVALID_ARG, leaf
    lf = np.ones(3, np.float32)
    for stride in (16, 18, 30):
        assert lib.lib().rsreg_voxel_grid(pts.ctypes.data, 1, stride, lf.ctypes.data, 1, 0, out.ctypes.data, C.byref(n_out), None) == lib.RSREG_ERR_INVALID_ARG
    assert lib.lib().rsreg_voxel_grid(pts.ctypes.data, 1, 32, lf.ctypes.data, 1, 0, out.ctypes.data, C.byref(n_out), None) == 0 and n_out.value == 1


def test_python_class_on_the_host(rs, lib):
    from rsreg_amd import api
    pts, leaf, _, _ = V.cases()["boundaries_aniso"]
    want, want_info = V.reference("boundaries_aniso")
    f = api.VoxelGrid()
    assert f.getDownsampleAllData() and f.getMinimumPointsNumberPerVoxel() == 0
    f.setLeafSize(*leaf)
    f.setInputCloud(rs.PointCloud(pts.copy(), is_dense=False))
    out = f.filter()
    assert out.points.tobytes() == want.tobytes() and (out.width, out.height, out.is_dense) == (len(want), 1, True)
    assert f.getMinBoxCoordinates().tolist() == want_info["min_b"] and f.getMaxBoxCoordinates().tolist() == want_info["max_b"]
    assert f.getNrDivisions().tolist() == want_info["div_b"] and f.getDivisionMultiplier().tolist() == want_info["divb_mul"]
    g = api.VoxelGrid()
    g.setLeafSize(0.25)
    assert g.getLeafSize().tolist() == [0.25] * 3
    # a leaf too small for the box: the output is the input, organized as it was
    pts2 = V.cases()["overflow_1291"][0]
    g.setLeafSize(1.0)
    g.setInputCloud(rs.PointCloud(pts2.copy(), width=5, height=2, is_dense=False))
    out2 = g.filter()
    assert g.info.overflowed == 1 and out2.points.tobytes() == pts2.tobytes() and (out2.width, out2.height, out2.is_dense) == (5, 2, False)
