"""GPU: the capture step on the device (csrc/depthcloud.hip: rsreg_cloud_from_depth, rsreg_cloud_from_depth_device) against the
host restatement (rsreg_depth_to_cloud) and the numpy reference (tests/depthcloud_ref.py): record bytes and the cloud's
n / stride / width / height / is_dense, equal, on every case of tests/depthcase_cases.py -- the CPU tests show what each case
covers.  And one registration of two clouds built this way, bit-identical to the same registration of uploaded records."""
import ctypes as C

import numpy as np
import pytest

import depthcase_cases as D
import depthcloud_ref as R

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


@pytest.mark.parametrize("device", [False, True], ids=["host_images", "device_images"])
@pytest.mark.parametrize("name", sorted(D.cases()))
def test_device_cloud_equals_host_and_reference(lib, ctx, name, device):
    case = D.cases()[name]
    want, want_meta, _ = D.reference(name)
    host, host_meta = D.run_host(lib, case)
    out = D.Handle(lib, ctx)
    got, meta, before, after = D.run_gpu(lib, ctx, case, out, device=device)
    out.close()
    assert meta == want_meta == host_meta
    same_bytes(got, want)
    same_bytes(got, host)
    assert after > before


def test_out_reused_across_sizes(lib, ctx):
    """one handle, a large cloud, a small one, the large one again: sizes, bytes and the version follow"""
    out = D.Handle(lib, ctx)
    versions = [out.version()]
    for name in ("ragged_67x131", "tiny_7x5_identity", "reference_13x7", "ragged_67x131"):
        got, meta, before, after = D.run_gpu(lib, ctx, D.cases()[name], out, device=(name == "reference_13x7"))
        want, want_meta, _ = D.reference(name)
        assert meta == want_meta and after == before + 1
        same_bytes(got, want)
        versions.append(after)
    assert versions == sorted(set(versions))
    out.close()


def test_second_context_gives_the_same_bytes(lib, ctx):
    from rsreg_amd import api
    other = api.Context(0)
    for name in ("distortion_both", "q2_zero"):
        want = D.reference(name)[0]
        for c in (other, ctx, other):
            out = D.Handle(lib, c)
            same_bytes(D.run_gpu(lib, c, D.cases()[name], out)[0], want)
            out.close()
    other.close()


@pytest.mark.parametrize("name", sorted(D.invalid()))
def test_refused_arguments(lib, ctx, name):
    p, dstride, cstride = D.invalid()[name]
    case = D.cases()["tiny_7x5_identity"]
    out = D.Handle(lib, ctx)
    D.run_gpu(lib, ctx, case, out)
    before, kept = out.version(), out.download()
    q = D.c_params(lib, p)
    rc = lib.lib().rsreg_cloud_from_depth(ctx.h, case.dbuf.ctypes.data, dstride, case.cbuf.ctypes.data, cstride, C.byref(q), out.h)
    assert rc == lib.RSREG_ERR_INVALID_ARG
    assert out.version() == before and out.info() == (35, 32, 7, 5, 0)      # refused: the cloud is as it was
    same_bytes(out.download(), kept)
    out.close()


def test_refused_handles_and_pointers(lib, ctx):
    from rsreg_amd import api
    case = D.cases()["tiny_7x5_identity"]
    q = D.c_params(lib, case.p)
    out = D.Handle(lib, ctx)
    other = api.Context(0)
    foreign = D.Handle(lib, other)
    f, g = lib.lib().rsreg_cloud_from_depth, lib.lib().rsreg_cloud_from_depth_device
    d, c = case.dbuf.ctypes.data, case.cbuf.ctypes.data
    assert f(ctx.h, d, case.dstride, c, case.cstride, C.byref(q), foreign.h) == lib.RSREG_ERR_INVALID_ARG      # a cloud of another context
    assert f(ctx.h, None, case.dstride, c, case.cstride, C.byref(q), out.h) == lib.RSREG_ERR_INVALID_ARG
    assert f(ctx.h, d, case.dstride, None, case.cstride, C.byref(q), out.h) == lib.RSREG_ERR_INVALID_ARG
    assert f(ctx.h, d, case.dstride, c, case.cstride, None, out.h) == lib.RSREG_ERR_INVALID_ARG
    assert f(ctx.h, d, case.dstride, c, case.cstride, C.byref(q), None) == lib.RSREG_ERR_INVALID_ARG
    assert g(ctx.h, None, case.dstride, None, case.cstride, C.byref(q), out.h) == lib.RSREG_ERR_INVALID_ARG
    assert out.version() == 0
    foreign.close()
    out.close()
    other.close()


def test_python_layer(rs, lib, ctx):
    from rsreg_amd import api
    case = D.cases()["distortion_both"]
    want, meta, _ = D.reference("distortion_both")
    f = api.DepthToCloud(ctx)
    f.setDepthIntrinsics(**D.intr_kw(case.p["depth"]))
    f.setColorIntrinsics(**D.intr_kw(case.p["color"]))
    f.setExtrinsics(case.p["rotation"], case.p["translation"])
    dev = f.compute(D.depth_view(case), D.color_view(case))
    assert dev.info() == (meta[0], 32, meta[2], meta[3], False)
    same_bytes(dev.download().points, want)
    # the images already in HBM, into the same cloud
    stamp = dev.stamp
    (dh, d_ptr), (ch, c_ptr) = D.device_bytes(lib, ctx, case.dbuf), D.device_bytes(lib, ctx, case.cbuf)
    again = api.DeviceCloud.from_depth_device(ctx, d_ptr, case.dstride, c_ptr, case.cstride, f.params((30, 40), (30, 40, 3)), out=dev)
    assert again is dev and dev.stamp[0] == stamp[0] and dev.stamp[1] == stamp[1] + 1
    same_bytes(dev.download().points, want)
    dh.close()
    ch.close()
    # padded host rows through DeviceCloud.from_depth
    case = D.cases()["padded_bpp4_bgr"]
    depth = np.lib.stride_tricks.as_strided(case.dbuf.view("<u2"), (12, 16), (case.dstride, 2))
    color = np.lib.stride_tricks.as_strided(case.cbuf, (12, 16, 4), (case.cstride, 4, 1))
    padded = api.DeviceCloud.from_depth(ctx, depth, color, api.depth_params(16, 12, color_bytes_per_pixel=4))
    same_bytes(padded.download().points, D.reference("padded_bpp4_bgr")[0])


@pytest.fixture(scope="module")
def two_frames(rs):
    """two rendered 250 x 200 frames as a camera would deliver them, and the numpy reference's records of each"""
    frames = []
    for k in (0, 1):
        depth, color, p = D.frame_images(rs.synth.render_frame(k, "50k", "parity"))
        rec, w, h, dense, _ = R.depth_to_cloud(depth, color, p)
        frames.append((depth, color, p, rs.PointCloud(rec.view(rs.POINT_DTYPE), width=w, height=h, is_dense=bool(dense))))
    return frames


def test_registration_of_built_clouds_is_bit_identical(rs, lib, ctx, two_frames):
    """from_depth clouds registered with the reference's ICP parameters give the 4 x 4 that the same records, uploaded with
    rsreg_cloud_upload, give: every bit, because the clouds are byte-equal; IntegralImageNormalEstimation takes the organized cloud"""
    from rsreg_amd import api
    built, uploaded = [], []
    for depth, color, p, ref_cloud in two_frames:
        dev = api.DeviceCloud.from_depth(ctx, depth, color, D.c_params(lib, p))
        assert dev.info() == (250 * 200, 32, 250, 200, False)
        same_bytes(dev.download().points, ref_cloud.points)
        built.append(dev)
        uploaded.append(api.DeviceCloud(ref_cloud, ctx=ctx))
    # the frames look like the renderer's: most pixels valid, some depth missing
    z = two_frames[0][3].points["z"]
    assert 0.05 < (z == 0).mean() < 0.5 and 0.5 < z[z > 0].min() and z.max() < 3.0

    def register(target, source):
        icp = api.IterativeClosestPoint(ctx)
        icp.params = api.icp_params(reference=True)
        icp.setInputSource(source)
        icp.setInputTarget(target)
        icp.align()
        return icp.getFinalTransformation(), icp.result

    T_built, r_built = register(built[0], built[1])
    T_up, r_up = register(uploaded[0], uploaded[1])
    assert T_built.tobytes() == T_up.tobytes()
    assert (r_built.converged, r_built.iterations, r_built.n_correspondences) == (r_up.converged, r_up.iterations, r_up.n_correspondences)
    assert r_built.converged and r_built.n_correspondences > 1000 and not np.array_equal(T_built, np.eye(4, dtype=np.float32))
    normals = built[0].integral_normals()
    assert normals.shape == (250 * 200, 4) and np.isfinite(normals[:, :3]).all(axis=1).mean() > 0.1
    np.testing.assert_array_equal(normals.view(np.uint32), uploaded[0].integral_normals().view(np.uint32))
