"""Every search and filter over cloud handles on every record layout: the same records at strides 12, 16, 20, 32 and 48 (20, 32, 36
and 48 where an entry point needs rgb at byte 16), uploaded through DeviceCloud with a np.void record type; whole records come back
through rsreg_cloud_download into raw bytes.  tests/layout_cases.py lays the records out: x, y, z first, every further word unique to
(record, word).

Every expected value comes from the numpy references (normals_ref, radius_ref, sor_ref, iinormals_ref, fpfh_ref) and, for
ApproximateVoxelGrid, from the sequential host filter, under the rules of the existing stride-32 tests: bit-equal where those are
bit-equal, tests/test_normals_gpu.py::_check_normals and tests/test_radius_gpu.py::_check_normals where they are not.  The results
at every stride are then byte-equal to the stride-32 result.

  * knn(10), knn_mean_distance(8), normals(10), radius_count(0.1), normals_radius(0.1) on the 60 x 50 "non_finite" cloud, and
    integral_normals() on the 250 x 200 rendered frame;
  * PassThrough (z, a range that removes about a third, negative and keep_organized both ways), StatisticalOutlierRemoval (mean_k 8,
    stddev 1.0, negative both ways), RadiusOutlierRemoval (r = 0.1, min_neighbors 2, keep_organized both ways): the kept set is the
    reference's, the output's stride is the input's, every byte of every kept record is the input record's, in input order; under
    keep_organized every word but the three NaN-ed ones is unchanged; width / height / is_dense as at stride 32; once, at stride
    48, in place;
  * FPFHEstimation with the cloud at strides 12 and 48 and the normals as 12-byte, 32-byte pcl::Normal and 48-byte records;
  * ApproximateVoxelGrid at strides 20, 36 (scalar loads) and 48 (the 16-byte load of csrc/voxel.hip), through
    rsreg_approx_voxel_grid_gpu and through the cloud-handle filter, on leaves of 1, 47, 48, 49, 1 023, 1 024, 1 025 and 5 000
    points: whole output records byte-equal to rsreg_approx_voxel_grid at the same stride, x, y, z, w, rgba equal to the stride-32 run;
  * ICP from raw device pointers that start 4 bytes into a 16-byte-aligned allocation, at strides 32 and 16: k_bbox takes its
    scalar branch at a stride that is a multiple of 16 (every other kernel that receives the pointer reads x, y, z as three floats
    through rec_xyz: csrc/icp_kernels.hpp, csrc/icp_dense.hpp, csrc/cellsort.hpp).
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import fpfh_ref as F
import iinormals_ref as II
import layout_cases as K
import normals_ref as N
import radius_ref as R
import sor_ref as S
from test_fpfh_gpu import _check_fpfh
from test_normals_gpu import _check_normals
from test_radius_gpu import _check_normals as _check_normals_radius

RADIUS = 0.1
Z_LO, Z_HI = 0.63, 1.2            # z is uniform in 0.4 .. 1.1: about a third lies below Z_LO
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    return api


@pytest.fixture(scope="module")
def ctx(api):
    t0 = time.perf_counter()
    yield api.Context(0)
    print("\ncloud layouts: %.1f s from the first context to the last test" % (time.perf_counter() - t0))


class _Xyz:
    """What _check_normals reads of a cloud."""

    def __init__(self, xyz):
        self.xyz = xyz

    def __len__(self):
        return len(self.xyz)


def _upload(api, ctx, xyz, stride, width=None, height=1, is_dense=False):
    dc = api.DeviceCloud(K.raw_cloud(xyz, stride, width, height, is_dense), ctx=ctx)
    assert dc.info() == (len(xyz), stride, len(xyz) if width is None else width, height, is_dense)
    return dc


def _download(dc):
    """(the records as (n, stride / 4) uint32, info) through rsreg_cloud_download into raw bytes."""
    from rsreg_amd import lib
    info = dc.info()
    n, stride = info[:2]
    buf = np.zeros((n, max(stride, 4) // 4), np.uint32)
    lib.check(lib.lib().rsreg_cloud_download(dc.h, buf.ctypes.data, n), dc.ctx.h)
    return buf, info


# ------------------------------------------------------------------------------------------------ references, once
@functools.lru_cache(maxsize=None)
def _ref_knn():
    return N.knn(K.non_finite_xyz(), 10)


@functools.lru_cache(maxsize=None)
def _ref_normals():
    return N.normals(K.non_finite_xyz(), 10, (0.0, 0.0, 0.0), knn_result=_ref_knn())


@functools.lru_cache(maxsize=None)
def _ref_mean():
    return S.knn_mean_distance(K.non_finite_xyz(), 8)


@functools.lru_cache(maxsize=None)
def _ref_search():
    return R.search(K.non_finite_xyz(), RADIUS)


@functools.lru_cache(maxsize=None)
def _ref_normals_radius():
    return R.normals(K.non_finite_xyz(), RADIUS, (0.0, 0.0, 0.0), nb=_ref_search())


@functools.lru_cache(maxsize=None)
def _frame_xyz():
    from rsreg_amd import synth
    fr = synth.render_frame(1, "50k")
    xyz = np.ascontiguousarray(fr.xyz)
    xyz.setflags(write=False)
    return xyz, fr.width, fr.height


@functools.lru_cache(maxsize=None)
def _frame_ref():
    xyz, w, h = _frame_xyz()
    return II.normals(xyz.reshape(h, w, 3))


_AT32 = {}   # the stride-32 results, made once each


# ------------------------------------------------------------------------------------------------ the searches
@pytest.mark.parametrize("stride", K.STRIDES)
def test_searches_at_every_stride(api, ctx, stride):
    xyz = K.non_finite_xyz()
    fin = S.finite_rows(xyz)
    cloud = _Xyz(xyz)

    def run(s):
        dc = _upload(api, ctx, xyz, s, 60, 50)
        idx, d2 = dc.knn(10)
        return {"idx": idx, "d2": d2, "mean": dc.knn_mean_distance(8), "normals": dc.normals(10), "count": dc.radius_count(RADIUS),
                "normals_radius": dc.normals_radius(RADIUS)}

    got = run(stride)
    want_idx, want_d2 = _ref_knn()
    assert (got["idx"] == want_idx).all() and (got["d2"].view(np.uint32) == want_d2.view(np.uint32)).all()
    assert (got["idx"][~fin] == -1).all() and (got["d2"][~fin] == 0).all()
    assert (got["mean"].view(np.uint32) == _ref_mean().view(np.uint32)).all() and (got["mean"][~fin] == 0).all()
    _check_normals(got["normals"], cloud, _ref_normals(), (0.0, 0.0, 0.0), True, "stride %d k=10" % stride)
    np.testing.assert_array_equal(got["count"], _ref_search().counts())
    assert got["count"].dtype == np.uint32 and (got["count"][~fin] == 0).all()
    _check_normals_radius(got["normals_radius"], cloud, _ref_normals_radius(), (0.0, 0.0, 0.0), True, "stride %d r=%g" % (stride, RADIUS))
    if "searches" not in _AT32:
        _AT32["searches"] = run(32)
    for key, val in got.items():
        assert val.tobytes() == _AT32["searches"][key].tobytes(), (key, stride)


@pytest.mark.parametrize("stride", K.STRIDES)
def test_integral_normals_at_every_stride(api, ctx, stride):
    """The rules of tests/test_iinormals_gpu.py::test_rendered_frame."""
    xyz, w, h = _frame_xyz()
    ref = _frame_ref()

    def run(s):
        dc = _upload(api, ctx, xyz, s, w, h)
        out, rect = dc.integral_normals_cloud(None, rect=True)
        info = out.info()
        rec = out.download_normals().points
        return rec.view(np.uint32).reshape(len(rec), 8), rect, info

    rec, rect, info = run(stride)
    assert info == (len(xyz), 32, w, h, False)
    assert (rect == ref.rect).all(), np.flatnonzero(rect != ref.rect)[:8]
    got_nan = rec[:, 0] == II.QNAN
    assert (got_nan == (rec[:, [0, 1, 2]] == II.QNAN).all(axis=1)).all()
    assert (got_nan == ~ref.has_normal).all()
    assert (rec[:, 4] == II.QNAN).all() and (rec[:, [3, 5, 6, 7]] == 0).all()
    clear = ref.has_normal & (ref.l >= 1e-12 * ref.gx2 * ref.gy2)
    left_out = 1.0 - clear[ref.has_normal].mean()
    n, n_ref = II.normal_vectors(rec), II.normal_vectors(ref.records)
    err = np.abs(n[clear].astype(np.float64) - n_ref[clear].astype(np.float64)).max()
    print("integral normals at stride %d: left out %.4f %%, max |n - n_ref| %.3g" % (stride, 100 * left_out, err))
    assert left_out <= 0.01
    assert err <= 2.0 ** -22
    assert float((~got_nan).mean()) == float(ref.has_normal.mean())
    if "iin" not in _AT32:
        _AT32["iin"] = run(32)
    assert rec.tobytes() == _AT32["iin"][0].tobytes() and (rect == _AT32["iin"][1]).all()


# ------------------------------------------------------------------------------------------------ the three filters
def _check_compact(src, out, keep, stride, dense):
    got, info = _download(out)
    kept = int(keep.sum())
    assert 0 < kept < len(src)
    assert info == (kept, stride, kept, 1, dense)
    assert got.shape == (kept, stride // 4) and got.tobytes() == src[keep].tobytes()       # every byte, in input order


def _check_organized(src, out, keep, stride, width, height):
    got, info = _download(out)
    assert 0 < int(keep.sum()) < len(src)
    assert info == (len(src), stride, width, height, False)                                 # something was removed
    assert got.shape == src.shape
    assert (got[:, 3:] == src[:, 3:]).all()                                                 # every word but x, y, z
    assert (got[keep, :3] == src[keep, :3]).all() and (got[~keep, :3] == K.QNAN).all()


def _passthrough(api, dc, negative, keep_organized, out=None):
    from rsreg_amd import lib
    out = out if out is not None else api.DeviceCloud(ctx=dc.ctx)
    lib.check(lib.lib().rsreg_cloud_passthrough(dc.ctx.h, dc.h, 2, Z_LO, Z_HI, int(negative), int(keep_organized), out.h), dc.ctx.h)
    return out


def _sor(api, dc, negative, out=None):
    from rsreg_amd import lib
    out = out if out is not None else api.DeviceCloud(ctx=dc.ctx)
    st = lib.SorStats()
    lib.check(lib.lib().rsreg_cloud_sor(dc.ctx.h, dc.h, 8, 1.0, int(negative), out.h, C.byref(st)), dc.ctx.h)
    return out, st


@functools.lru_cache(maxsize=None)
def _ref_sor(negative):
    keep, dist, stats = S.sor(K.non_finite_xyz(), 8, 1.0, negative)
    assert S.threshold_margin(dist, K.non_finite_xyz(), stats[3]) > 1e-9   # no distance at the threshold: the kept set is the reference's
    return keep, stats


@pytest.mark.parametrize("dense_in", [False, True])
@pytest.mark.parametrize("stride", K.STRIDES)
def test_filters_at_every_stride(api, ctx, stride, dense_in):
    xyz = K.non_finite_xyz()
    src = K.words(xyz, stride)
    dc = _upload(api, ctx, xyz, stride, 60, 50, dense_in)
    for negative in (False, True):
        keep = S.passthrough_keep(xyz, 2, Z_LO, Z_HI, negative)
        if not negative:
            assert 0.25 < 1.0 - keep[S.finite_rows(xyz)].mean() < 0.4                        # about a third goes
        _check_compact(src, _passthrough(api, dc, negative, False), keep, stride, True)     # PassThrough's output is dense
        _check_organized(src, _passthrough(api, dc, negative, True), keep, stride, 60, 50)
        keep, (n_valid, mean, stddev, thr) = _ref_sor(negative)
        out, st = _sor(api, dc, negative)
        assert st.n_valid == n_valid and st.n_kept == int(keep.sum())
        for a, b in ((st.mean, mean), (st.stddev, stddev), (st.threshold, thr)):
            assert abs(a - b) <= 1e-12 * abs(b)
        _check_compact(src, out, keep, stride, dense_in)
    counts = _ref_search().counts()
    for negative in (False, True):
        keep = R.ror_keep(counts, 2, negative)
        out, kept = dc.radius_outlier_removal(RADIUS, 2, negative)
        assert kept == int(keep.sum())
        _check_compact(src, out, keep, stride, dense_in)
        out, kept = dc.radius_outlier_removal(RADIUS, 2, negative, keep_organized=True)
        assert kept == int(keep.sum())
        _check_organized(src, out, keep, stride, 60, 50)
    assert (_download(dc)[0] == src).all()                                                   # the input is as it was


def test_filters_in_place_at_stride_48(api, ctx):
    xyz = K.non_finite_xyz()
    src = K.words(xyz, 48)
    dc = _upload(api, ctx, xyz, 48, 60, 50)
    assert _passthrough(api, dc, False, False, out=dc) is dc
    _check_compact(src, dc, S.passthrough_keep(xyz, 2, Z_LO, Z_HI), 48, True)
    dc = _upload(api, ctx, xyz, 48, 60, 50)
    _passthrough(api, dc, True, True, out=dc)
    _check_organized(src, dc, S.passthrough_keep(xyz, 2, Z_LO, Z_HI, True), 48, 60, 50)
    dc = _upload(api, ctx, xyz, 48, 60, 50)
    _sor(api, dc, False, out=dc)
    _check_compact(src, dc, _ref_sor(False)[0], 48, False)
    counts = _ref_search().counts()
    dc = _upload(api, ctx, xyz, 48, 60, 50)
    same, kept = dc.radius_outlier_removal(RADIUS, 2, out=dc)
    assert same is dc and kept == int(R.ror_keep(counts, 2).sum())
    _check_compact(src, dc, R.ror_keep(counts, 2), 48, False)
    dc = _upload(api, ctx, xyz, 48, 60, 50)
    dc.radius_outlier_removal(RADIUS, 2, keep_organized=True, out=dc)
    _check_organized(src, dc, R.ror_keep(counts, 2), 48, 60, 50)


# ------------------------------------------------------------------------------------------------ FPFH
@functools.lru_cache(maxsize=None)
def _ref_fpfh():
    """(the reference's float32 normals at k = 10, NaN for a non-finite record; its curvatures; fpfh_ref at k = 10 over them)"""
    ref = _ref_normals()
    nrm = np.ascontiguousarray(ref.normal, np.float32)
    return nrm, ref.curvature, F.fpfh(K.non_finite_xyz(), nrm, 10)


def _normal_records(api, nrm, curvature, stride):
    if stride == 32:                                          # pcl::Normal
        rec = np.zeros(len(nrm), api.NORMAL_DTYPE)
        rec["normal_x"], rec["normal_y"], rec["normal_z"], rec["curvature"] = nrm[:, 0], nrm[:, 1], nrm[:, 2], curvature
        return rec
    return K.records(nrm, stride)                             # three floats, then words of their own


def test_fpfh_cloud_and_normals_layouts(api, ctx):
    xyz = K.non_finite_xyz()
    nrm, curvature, ref = _ref_fpfh()
    assert (ref.nan_rows == ~S.finite_rows(xyz)).all() and ref.nan_rows.any()
    first = None
    for stride in (12, 48, 32):
        dc = _upload(api, ctx, xyz, stride, 60, 50)
        for nstride in (12, 32, 48):
            normals = api.DeviceCloud(K.RawCloud(_normal_records(api, nrm, curvature, nstride), 60, 50, False), ctx=ctx)
            assert normals.info()[:2] == (len(xyz), nstride)
            out = dc.fpfh_cloud(normals, 10)
            assert out.info() == (len(xyz), 132, 60, 50, False)
            got = out.download_fpfh().points["histogram"]
            _check_fpfh(got, ref, "fpfh: cloud stride %d, normals stride %d" % (stride, nstride))
            assert (got.view(np.uint32)[ref.nan_rows] == K.QNAN).all()
            spfh = dc.spfh(normals, 10)
            np.testing.assert_array_equal(spfh[~ref.fragile], ref.spfh[~ref.fragile])
            both = got.tobytes() + spfh.tobytes()
            first = both if first is None else first
            assert both == first, (stride, nstride)


# ------------------------------------------------------------------------------------------------ ApproximateVoxelGrid
@functools.lru_cache(maxsize=None)
def _voxel_host(stride):
    """rsreg_approx_voxel_grid, the sequential host filter, at this stride: (n_out, stride / 4) uint32."""
    from rsreg_amd import lib
    src = K.words(K.voxel_xyz(), stride)
    out = np.zeros_like(src)
    n_out = C.c_size_t(0)
    leaf = np.full(3, K.VOXEL_LEAF, np.float32)
    lib.check(lib.lib().rsreg_approx_voxel_grid(src.ctypes.data, len(src), stride, leaf.ctypes.data, out.ctypes.data, C.byref(n_out)))
    return out[:n_out.value].copy()


@pytest.mark.parametrize("stride", [20, 36, 48])
def test_approximate_voxel_grid_layouts(api, ctx, stride):
    from rsreg_amd import lib
    L = lib.lib()
    xyz = K.voxel_xyz()
    src = K.words(xyz, stride)
    leaf = np.full(3, K.VOXEL_LEAF, np.float32)
    want = _voxel_host(stride)
    assert len(xyz) == sum(K.LEAF_POINTS) + K.VOXEL_HOLES
    assert len(want) == len(K.LEAF_POINTS)                    # one run per leaf: every run class, both sides of kLongRun and kHugeRun
    assert (want[:, 3] == np.float32(1.0).view(np.uint32)).all() and (want[:, 5:] == 0).all()
    out = np.full_like(src, 0xdeadbeef)
    n_out = C.c_size_t(0)
    lib.check(L.rsreg_approx_voxel_grid_gpu(ctx.h, src.ctypes.data, len(src), stride, leaf.ctypes.data, out.ctypes.data, C.byref(n_out)), ctx.h)
    assert n_out.value == len(want) and out[:len(want)].tobytes() == want.tobytes()
    assert (out[len(want):] == 0xdeadbeef).all()              # nothing behind the output was written
    dc = _upload(api, ctx, xyz, stride)
    filt = api.DeviceCloud(ctx=ctx)
    lib.check(L.rsreg_cloud_filter(ctx.h, dc.h, leaf.ctypes.data, filt.h), ctx.h)
    got, info = _download(filt)
    assert info[:2] == (len(want), stride) and got.tobytes() == want.tobytes()
    assert (want[:, :5] == _voxel_host(32)[:, :5]).all()      # x, y, z, w, rgba: the stride-32 run
    if "voxel" not in _AT32:
        d32, f32 = _upload(api, ctx, xyz, 32), api.DeviceCloud(ctx=ctx)
        lib.check(L.rsreg_cloud_filter(ctx.h, d32.h, leaf.ctypes.data, f32.h), ctx.h)
        _AT32["voxel"] = _download(f32)[0]
        assert _AT32["voxel"].tobytes() == _voxel_host(32).tobytes()
    assert (got[:, :5] == _AT32["voxel"][:, :5]).all()


# ------------------------------------------------------------------------------------------------ ICP from an unaligned raw pointer
def test_icp_raw_pointer_off_the_16_byte_boundary(api, ctx):
    """The same target and source as 32-byte and as 16-byte records that start 4 bytes into a 16-byte-aligned allocation: the bytes
    of the 4 x 4 and the number of correspondences are those of the aligned run."""
    from rsreg_amd import lib, synth
    L = lib.lib()
    tgt, src = synth.render_frame(0, "50k", "parity"), synth.render_frame(1, "50k", "parity")
    guess = np.ascontiguousarray(synth.small_transform(0.3, (0.002, -0.001, 0.003)).astype(np.float32).T)
    prm = api.icp_params(max_iterations=3, criteria_mode=1, pipeline_mode=2, max_correspondence_distance=0.03)
    holder = api.Context(0)                                   # the records live in clouds of ANOTHER context: bare addresses go in

    def put(recs, stride, shift):
        """The records in HBM, `shift` bytes into an allocation: (handle, address of the first record)."""
        raw = np.zeros((len(recs) + (1 if shift else 0)) * stride, np.uint8)
        raw[shift:shift + len(recs) * stride] = recs.reshape(-1).view(np.uint8)
        h = C.c_void_p()
        lib.check(L.rsreg_cloud_create(holder.h, C.byref(h)), holder.h)
        lib.check(L.rsreg_cloud_upload(h, raw.ctypes.data, len(raw) // stride, stride, len(raw) // stride, 1, 0), holder.h)
        base = int(L.rsreg_cloud_device_ptr(h))
        assert base % 16 == 0
        return h, base + shift

    got = {}
    for stride in (32, 16):
        t, s = K.words(tgt.xyz, stride), K.words(src.xyz, stride)
        for shift in (0, 4):
            (ht, pt), (hs, ps) = put(t, stride, shift), put(s, stride, shift)
            assert pt % 16 == shift and ps % 16 == shift
            run = api.Context(0)
            res = lib.IcpResult()
            out = np.zeros((len(s), stride // 4), np.float32)
            lib.check(L.rsreg_icp_set_source_device(run.h, C.c_void_p(ps), len(s), stride, 0), run.h)
            lib.check(L.rsreg_icp_set_target_device(run.h, C.c_void_p(pt), len(t), stride, 0, 0.03), run.h)
            lib.check(L.rsreg_icp_align(run.h, guess.ctypes.data, C.byref(prm), C.byref(res), out.ctypes.data, stride), run.h)
            got[(stride, shift)] = (bytes(bytearray(res.transform)), int(res.n_correspondences), int(res.iterations), out[:, :3].tobytes())
            run.close()
            for h in (ht, hs):
                L.rsreg_cloud_destroy(h)
    ref = got[(32, 0)]
    assert ref[1] > 0.5 * len(src) and ref[2] == 3
    for key, val in got.items():
        assert val == ref, key
