"""GPU: the two voxel filters of csrc/voxel.hip across the float32 range, byte for byte against their references
(tests/approx_voxel_ref.py, tests/voxelgrid_ref.py) and their sequential host restatements.  tests/voxel_scale_cases.py holds the
clouds; tests/test_voxel_scale_cpu.py shows on the references alone what each of them is there for, and that 2^-100 .. 2^100 is a
window in which scaling the cloud and the leaf commutes with both filters.

  * ApproximateVoxelGrid on (a) scaled clouds, (b) cell indices at and past int32, (c) cancelling runs, (d) sums that leave the normal
    range: rsreg_approx_voxel_grid_gpu and rsreg_cloud_filter; rsreg_cloud_filter_async (the side scratch set) on two of them.
  * VoxelGrid on (a), (d) and (e) far and wide boxes: rsreg_voxel_grid_gpu and rsreg_cloud_voxel_grid, records, info and cloud meta.
  * Inside the window the scaled and the scale-1 call run in the same test and are compared with each other, moved by 2^e.
  * Strides 20 and 48 (the scalar and the 16-byte loads) on a case of (b) and of (e); an extreme case from a fresh context that has
    filtered a metre-scale frame first.
No tolerance anywhere: every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import voxel_scale_cases as S
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


def approx_both(lib, ctx, pts, leaf):
    """the two synchronous entry points; they must agree with each other before they are compared with anything else"""
    got = S.approx_gpu_host_records(lib, ctx, pts, leaf)
    cloud, meta = S.approx_gpu_cloud(lib, ctx, pts, leaf)
    same_bytes(cloud, got)
    assert meta == (len(got), pts.dtype.itemsize, len(got), 1, 0)
    return got


def grid_both(lib, ctx, pts, leaf, all_data, mp, want_info, n_want):
    got, info = V.run_gpu_host_records(lib, ctx, pts, leaf, all_data, mp)
    cloud, cloud_info, meta, (before, after) = V.run_gpu_cloud(lib, ctx, pts, leaf, all_data, mp, is_dense=0)
    assert info == want_info and cloud_info == want_info
    same_bytes(cloud, got)
    if want_info["overflowed"]:
        assert meta == (len(pts), pts.dtype.itemsize, len(pts), 1, 0)
    else:
        assert meta == (n_want, pts.dtype.itemsize, n_want, 1, 1)
    assert after > before
    return got


# ------------------------------------------------------------------------------------------------ ApproximateVoxelGrid
@pytest.mark.parametrize("case", [c for c in S.APPROX_ALL if c[2] == 0], ids=S.label)
def test_approx_equals_reference_and_host(lib, ctx, case):
    pts, leaf = S.approx_case(*case)
    want = S.approx_reference(*case)
    got = approx_both(lib, ctx, pts, leaf)
    same_bytes(got, want)
    same_bytes(got, S.approx_host(lib, pts, leaf))


@pytest.mark.parametrize("name,e", [(n, e) for n in S.SCALED for e in S.EXPONENTS])
def test_approx_commutes_with_powers_of_two(lib, ctx, name, e):
    pts0, leaf0 = S.scaled(name, 0)
    ptse, leafe = S.scaled(name, e)
    got0, gote = approx_both(lib, ctx, pts0, leaf0), approx_both(lib, ctx, ptse, leafe)
    same_bytes(gote, S.moved(got0, e))
    same_bytes(gote, S.approx_reference("scaled", name, e))
    same_bytes(gote, S.approx_host(lib, ptse, leafe))


@pytest.mark.parametrize("name", ["cancel_1500_window_ends_at_zero", "cell_l1_xyz"])
def test_approx_on_the_side_scratch_set(lib, ctx, name):
    """rsreg_cloud_filter_async: the same kernels on a scratch set and a stream of their own; twice, so that both sets of a worker run"""
    pts, leaf = S.approx_cases()[name]
    want = S.approx_reference("cell", name)
    for _ in range(2):
        got, meta = S.approx_gpu_cloud(lib, ctx, pts, leaf, asynchronous=True)
        same_bytes(got, want)
        assert meta == (len(want), 32, len(want), 1, 0)


# ------------------------------------------------------------------------------------------------ VoxelGrid
@pytest.mark.parametrize("case", [c for c in S.GRID_ALL if c[2] == 0], ids=S.label)
def test_grid_equals_reference_and_host(lib, ctx, case):
    pts, leaf, all_data, mp = S.grid_case(*case)
    want, want_info = S.grid_reference(*case)
    got = grid_both(lib, ctx, pts, leaf, all_data, mp, want_info, len(want))
    same_bytes(got, want)
    host, host_info = V.run_host(lib, pts, leaf, all_data, mp)
    assert host_info == want_info
    same_bytes(got, host)


@pytest.mark.parametrize("name,e", [(n, e) for n in S.SCALED for e in S.EXPONENTS])
def test_grid_commutes_with_powers_of_two(lib, ctx, name, e):
    pts0, leaf0 = S.scaled(name, 0)
    ptse, leafe = S.scaled(name, e)
    want, want_info = S.grid_reference("scaled", name, e)
    assert want_info == S.grid_reference("scaled", name, 0)[1]
    got0 = grid_both(lib, ctx, pts0, leaf0, 1, 0, want_info, len(want))
    gote = grid_both(lib, ctx, ptse, leafe, 1, 0, want_info, len(want))
    same_bytes(gote, S.moved(got0, e))
    same_bytes(gote, want)


def test_grid_refuses_leaves_whose_reciprocal_is_not_finite(lib, ctx):
    pts = S.grid_cases()["far_1e9"][0]
    h, out = V.Handle(lib, ctx, pts), V.Handle(lib, ctx)
    src, dst, n_out = R.raw_copy(pts), np.zeros_like(pts), C.c_size_t(0)
    for leaf in S.REFUSED_LEAVES:
        for lf in ((leaf, 1.0, 1.0), (1.0, 1.0, leaf)):
            p = V.params(lib, lf, 1, 0)
            assert lib.lib().rsreg_cloud_voxel_grid(ctx.h, h.h, C.byref(p), out.h, None) == lib.RSREG_ERR_INVALID_ARG
            assert lib.lib().rsreg_voxel_grid_gpu(ctx.h, src.ctypes.data, len(src), 32, C.byref(p), dst.ctypes.data, C.byref(n_out),
                                                  None) == lib.RSREG_ERR_INVALID_ARG
    h.close()
    out.close()


# ------------------------------------------------------------------------------------------------ strides and contexts
@pytest.mark.parametrize("dtype", [S.POINT20, V.POINT48], ids=["stride20", "stride48"])
def test_strides(lib, ctx, dtype):
    """a case of (b) and a case of (e) as 20-byte records (scalar loads in vox_load and k_vg_keys) and as 48-byte records (16-byte loads)"""
    pts, leaf = S.approx_cases()["cell_l1_x"]
    want = S.approx_reference("cell", "cell_l1_x")
    rec = S.restride(pts, dtype)
    got = approx_both(lib, ctx, rec, leaf)
    assert S.same_fields(got, want)
    same_bytes(got, S.approx_host(lib, rec, leaf))
    if "extra" in dtype.names:
        assert (got["extra"] == 0).all()
    for name in ("far_plus_3e9_nan", "far_max_b_only_y"):
        pts, leaf, all_data, mp = S.grid_cases()[name]
        want, want_info = S.grid_reference("far", name)
        rec = S.restride(pts, dtype)
        got = grid_both(lib, ctx, rec, leaf, all_data, mp, want_info, len(want))
        assert S.same_fields(got, want)
        same_bytes(got, V.run_host(lib, rec, leaf, all_data, mp)[0])
        if "extra" in dtype.names:
            assert (got["extra"] == 0).all()


def test_fresh_context_after_a_metre_scale_frame(rs, lib):
    """the scratch of a context that has filtered a rendered frame (both filters) holds that frame's keys and sums; the extreme
    cases that follow must not see them"""
    from rsreg_amd import api
    other = api.Context(0)
    frame = R.raw_copy(rs.synth.render_frame(0, "50k", "parity").points)
    assert len(approx_both(lib, other, frame, (0.05, 0.05, 0.05))) > 100
    assert V.run_gpu_cloud(lib, other, frame, (0.05, 0.05, 0.05), 1, 0, is_dense=0)[1]["n_leaves"] > 100
    for name in ("cell_l1_y", "cancel_1500"):
        pts, leaf = S.approx_cases()[name]
        same_bytes(approx_both(lib, other, pts, leaf), S.approx_reference("cell", name))
    for name in ("far_minus_3e9_min2", "last_division_rounds_up_nan"):
        pts, leaf, all_data, mp = S.grid_cases()[name]
        want, want_info = S.grid_reference("far", name)
        same_bytes(grid_both(lib, other, pts, leaf, all_data, mp, want_info, len(want)), want)
    other.close()
