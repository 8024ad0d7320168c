"""rsreg_cloud_integral_normals (pcl::IntegralImageNormalEstimation, AVERAGE_3D_GRADIENT) on the GPU, the Python and C++
adaptors, against tests/iinormals_ref.py.

The window sizes (rect_out: the depth-change map, the two chamfer passes, the truncation) are EQUAL to the reference's on every
input.  The normals are byte-equal where every window sum is exact (coordinates that are multiples of 2^-12).  On a rendered
frame, where the reference's l >= 1e-12 |gx|^2 |gy|^2, they are within 2^-22: rounding a unit vector to float moves a component
by at most 2^-25 of 1 (2^-24 relative), and the two f64 sums differ by their order -- the reference takes them from a table,
the kernel adds the window's elements -- about 1e-11 relative; the bound is four times the first term.  The share of records
that condition leaves out is at most 1 %, asserted on the reference alone (measured: 0 %), and the share of records with a
normal equals the reference's (0.5198 on this frame).
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import iinormals_cases as K
import iinormals_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 8                      # csrc/iinormals_kernels.hpp: kIinBand, the rows a workgroup of a chamfer pass owns
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


def _cloud(P, seed=0):
    """An organized cloud of the (h, w, 3) array: a colour and a w of their own each, which must not enter a result."""
    from rsreg_amd import POINT_DTYPE, PointCloud
    h, w, _ = P.shape
    rng = np.random.default_rng(seed)
    pts = np.zeros(w * h, POINT_DTYPE)
    flat = P.reshape(-1, 3)
    pts["x"], pts["y"], pts["z"] = flat[:, 0], flat[:, 1], flat[:, 2]
    pts["w"] = rng.random(w * h).astype(np.float32)
    pts["rgba"] = rng.integers(0, 2 ** 32, w * h, dtype=np.uint32)
    return PointCloud(pts, width=w, height=h, is_dense=False)


def _run(api, ctx, cloud, **params):
    """(records as (n, 8) uint32, rect, the output cloud's info)"""
    dc = api.DeviceCloud(cloud, ctx=ctx)
    out, rect = dc.integral_normals_cloud(api.iin_params(**params) if params else None, rect=True)
    info = out.info()
    rec = out.download_normals().points
    out.close()
    dc.close()
    return rec.view(np.uint32).reshape(len(rec), 8), rect, info


@functools.lru_cache(maxsize=None)
def _quantised():
    return K.quantised_cloud()


@functools.lru_cache(maxsize=None)
def _quantised_ref(s):
    return R.normals(_quantised(), smoothing=s)


@functools.lru_cache(maxsize=None)
def _frame():
    from rsreg_amd import synth
    return synth.render_frame(1, "50k")


@functools.lru_cache(maxsize=None)
def _frame_ref():
    fr = _frame()
    return R.normals(fr.xyz.reshape(fr.height, fr.width, 3))


# ------------------------------------------------------------------------------------------------ 1. exact sums
@pytest.mark.parametrize("s", [10.0, 3.5, 31.0])
def test_quantised_cloud_bytes(api, ctx, s):
    P = _quantised()
    ref = _quantised_ref(s)
    rec, rect, info = _run(api, ctx, _cloud(P), normal_smoothing_size=s)
    print("quantised, s = %g: records with a window %d, with a normal %d, window sizes %s" %
          (s, int((ref.rect > 0).sum()), int(ref.has_normal.sum()), np.unique(ref.rect).tolist()))
    assert info == (96 * 64, 32, 96, 64, False)
    assert (rect == ref.rect).all(), np.flatnonzero(rect != ref.rect)[:8]
    bad = np.flatnonzero((rec != ref.records).any(axis=1))
    assert len(bad) == 0, (bad[:4], rec[bad[:4]], ref.records[bad[:4]])
    assert ref.has_normal.any() and (ref.rect == 0).any()


# ------------------------------------------------------------------------------------------------ 2. bands and halos
def _boundary_rows(h):
    return [r for b in range(BAND, h, BAND) for r in (b - 1, b)]


@pytest.mark.parametrize("w,h", [(65, 47), (129, 70), (100, 12 * BAND + 1)])
@pytest.mark.parametrize("s", [10.0, 40.0])
def test_pass_band_and_halo_edges(api, ctx, w, h, s):
    P = K.spike_frame(w, h, _boundary_rows(h))
    z = P[..., 2]
    D = R.distance_map(R.depth_change_map(z, 0.02))
    want = R.rect_map(z, D, s).reshape(-1)
    _, rect, _ = _run(api, ctx, _cloud(P), normal_smoothing_size=s)
    print("spikes %d x %d, s = %g: windows %d, sizes %s" % (w, h, s, int((want > 0).sum()), np.unique(want).tolist()))
    assert (rect == want).all(), np.flatnonzero(rect != want)[:8]
    if w > 2 * int(s) and h > 2 * int(s):
        assert (want > 0).any() and len(np.unique(want)) >= 3


def test_far_zero_reaches_through_many_bands(api, ctx):
    """One depth change in a flat 90 x 90 frame: the distances grow past every band and halo to s = 40 and beyond."""
    P = K.spike_frame(90, 90, [])
    P[..., 2] = 1.0
    P[3, 85, 2] = 2.0
    for s in (10.0, 40.0, 64.0):
        z = P[..., 2]
        want = R.rect_map(z, R.distance_map(R.depth_change_map(z, 0.02)), s).reshape(-1)
        _, rect, _ = _run(api, ctx, _cloud(P), normal_smoothing_size=s)
        assert (rect == want).all(), (s, np.flatnonzero(rect != want)[:8])


# ------------------------------------------------------------------------------------------------ 3. degenerate shapes
def test_degenerate_shapes(api, ctx):
    from rsreg_amd import lib
    L = lib.lib()
    P = K.plane_frame(21, 30, 0.25, -0.5, 2.0)                      # w = 2 B + 1: one interior column
    ref = R.normals(P)
    rec, rect, info = _run(api, ctx, _cloud(P))
    assert (rect == ref.rect).all() and rec.tobytes() == ref.records.tobytes()
    assert (np.flatnonzero(rect) % 21 == 10).all() and (rect > 0).sum() == 10 and ref.has_normal.sum() == 10
    P = K.plane_frame(20, 30, 0.25, -0.5, 2.0)                      # w = 2 B: nothing has a normal; not an error
    rec, rect, info = _run(api, ctx, _cloud(P))
    assert not rect.any() and (rec[:, [0, 1, 2, 4]] == R.QNAN).all() and (rec[:, [3, 5, 6, 7]] == 0).all()
    assert info == (600, 32, 20, 30, False)
    # refused, `out` untouched
    dc = api.DeviceCloud(_cloud(K.plane_frame(40, 30, 0.25, -0.5, 2.0)), ctx=ctx)
    out = api.DeviceCloud(_cloud(K.plane_frame(5, 4, 0.0, 0.0, 1.0)), ctx=ctx)
    before, stamp = out.download().points.tobytes(), out.stamp
    inv = lib.RSREG_ERR_INVALID_ARG
    flat = _cloud(K.plane_frame(40, 30, 0.25, -0.5, 2.0))
    flat.width, flat.height = 1200, 1
    unorganized = api.DeviceCloud(flat, ctx=ctx)
    call = lambda cloud, **kw: L.rsreg_cloud_integral_normals(ctx.h, cloud.h, C.byref(api.iin_params(**kw)), out.h, None)
    assert call(unorganized) == inv
    assert call(dc, method=0) == inv and call(dc, method=2) == inv and call(dc, method=3) == inv
    assert call(dc, normal_smoothing_size=0.0) == inv and call(dc, normal_smoothing_size=65.0) == inv
    assert call(dc, normal_smoothing_size=float("nan")) == inv
    assert call(dc, depth_dependent_smoothing=1) == inv
    assert call(dc, border_policy=1) == inv
    assert call(dc, max_depth_change_factor=-0.1) == inv and call(dc, max_depth_change_factor=float("inf")) == inv
    assert L.rsreg_cloud_integral_normals(ctx.h, dc.h, None, dc.h, None) == inv        # out == in
    assert L.rsreg_cloud_integral_normals(ctx.h, dc.h, None, None, None) == inv
    foreign = api.DeviceCloud(ctx=api.Context(0))
    assert L.rsreg_cloud_integral_normals(ctx.h, dc.h, None, foreign.h, None) == inv   # a cloud of another context
    assert out.download().points.tobytes() == before and out.stamp == stamp
    with pytest.raises(lib.RsregError) as e:
        dc.integral_normals(api.iin_params(method=0))
    assert e.value.status == inv
    assert call(dc, normal_smoothing_size=64.0) == 0 and out.info()[:4] == (1200, 32, 40, 30) and out.stamp[1] != stamp[1]
    assert L.rsreg_version() == 4


# ------------------------------------------------------------------------------------------------ 4. a rendered frame
def test_rendered_frame(api, ctx):
    fr, ref = _frame(), _frame_ref()
    rec, rect, info = _run(api, ctx, fr)
    assert info == (len(fr), 32, fr.width, fr.height, False)
    assert (rect == ref.rect).all(), np.flatnonzero(rect != ref.rect)[:8]
    got_nan = rec[:, 0] == R.QNAN
    assert (got_nan == (rec[:, [0, 1, 2]] == R.QNAN).all(axis=1)).all()
    assert (got_nan == ~ref.has_normal).all()
    assert (rec[:, 4] == R.QNAN).all() and (rec[:, [3, 5, 6, 7]] == 0).all()
    clear = ref.has_normal & (ref.l >= 1e-12 * ref.gx2 * ref.gy2)
    left_out = 1.0 - clear[ref.has_normal].mean()
    n, n_ref = R.normal_vectors(rec), R.normal_vectors(ref.records)
    err = np.abs(n[clear].astype(np.float64) - n_ref[clear].astype(np.float64)).max()
    share, share_ref = float((~got_nan).mean()), float(ref.has_normal.mean())
    print("rendered 50k frame: normals on %.4f of the records (reference %.4f), left out %.4f %%, max |n - n_ref| %.3g, window sizes %s" %
          (share, share_ref, 100 * left_out, err, np.bincount(ref.rect).tolist()))
    assert left_out <= 0.01
    assert err <= 2.0 ** -22
    assert share == share_ref and 0.4 < share_ref < 0.65
    four, rect2 = api.DeviceCloud(fr, ctx=ctx).integral_normals(rect=True)
    assert four.shape == (len(fr), 4) and four.dtype == np.float32 and (rect2 == rect).all()
    assert four.view(np.uint32).tobytes() == rec[:, [0, 1, 2, 4]].tobytes()


# ------------------------------------------------------------------------------------------------ 5. the same bytes elsewhere
def test_same_bytes_on_another_context_and_after_other_work(api, ctx):
    fr = _frame()
    vp = (0.3, -0.2, 5.0)
    want, want_rect, _ = _run(api, ctx, fr, viewpoint=vp)
    plain, _, _ = _run(api, ctx, fr)
    flipped = (want[:, :3] != plain[:, :3]).any(axis=1)
    assert flipped.any() and not flipped.all()                     # the viewpoint reaches the kernel
    other = api.Context(0)
    got, rect, _ = _run(api, other, _cloud(_quantised()), normal_smoothing_size=3.5)   # (a smaller frame first: scratch grows)
    got, rect, _ = _run(api, other, fr, viewpoint=vp)
    assert got.tobytes() == want.tobytes() and (rect == want_rect).all()
    # the k-NN normals and an alignment use the context's index and scratch; then the same call again
    src = _frame()
    from rsreg_amd import synth
    tgt = synth.render_frame(0, "50k")
    api.DeviceCloud(tgt, ctx=other).normals(10)
    icp = api.IterativeClosestPoint(ctx=other)
    icp.setInputSource(src)
    icp.setInputTarget(tgt)
    icp.align()
    got, rect, _ = _run(api, other, fr, viewpoint=vp)
    assert got.tobytes() == want.tobytes() and (rect == want_rect).all()


def test_adaptors(api, ctx, tmp_path):
    """tests/cpp/iinormals_runner.cpp gives the bytes of the Python path, from host clouds and from device clouds; so does
    api.IntegralImageNormalEstimation on a host cloud and on a device cloud."""
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "iinormals_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "iinormals_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    fr = _frame()
    vp = (0.3, -0.2, 5.0)
    want = api.DeviceCloud(fr, ctx=ctx).integral_normals_cloud(api.iin_params(viewpoint=vp, normal_smoothing_size=7.5,
                                                                              max_depth_change_factor=0.03)).download_normals()
    ne = api.IntegralImageNormalEstimation()
    ne.setNormalEstimationMethod(ne.AVERAGE_3D_GRADIENT)
    ne.setMaxDepthChangeFactor(0.03)
    ne.setNormalSmoothingSize(7.5)
    ne.setViewPoint(*vp)
    ne.setInputCloud(fr)                                     # a host cloud: through a temporary DeviceCloud
    host = ne.compute()
    assert host.points.tobytes() == want.points.tobytes()
    assert (host.width, host.height, host.is_dense) == (fr.width, fr.height, False) == (want.width, want.height, want.is_dense)
    ne.setInputCloud(api.DeviceCloud(fr, ctx=ctx))
    assert ne.compute().download_normals().points.tobytes() == want.points.tobytes()
    fr.points.tofile(str(tmp_path / "in.bin"))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(fr.width), str(fr.height), "0.03", "7.5", "0.3", "-0.2", "5", str(tmp_path / "host.bin"),
                        str(tmp_path / "dev.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    vals = dict(l.split() for l in r.stdout.strip().splitlines())
    for name in ("host.bin", "dev.bin"):
        assert open(str(tmp_path / name), "rb").read() == want.points.tobytes()
    assert int(vals["size"]) == int(vals["size_device"]) == len(fr) and int(vals["width"]) == fr.width and int(vals["height"]) == fr.height
    assert vals["dense"] == vals["dense_device"] == "0"


# ------------------------------------------------------------------------------------------------ 6. the consumer
def test_plane_sums_from_the_device_cloud_and_from_the_download(api):
    """Point-to-plane ICP on the 50 k pair with the target's integral-image normals, handed over as the device cloud and
    downloaded through rsreg_icp_set_target_normals: the 32 sums of the first search are the same doubles, and a NaN normal
    leaves its pair out of the plane terms only."""
    from rsreg_amd import lib, synth
    L = lib.lib()
    tgt, src = synth.render_frame(0, "50k"), synth.render_frame(1, "50k")
    t, s = np.ascontiguousarray(tgt.points), np.ascontiguousarray(src.points)
    prm = api.icp_params(max_correspondence_distance=0.05, estimation=lib.ESTIMATION_POINT_TO_PLANE_LLS)
    sums = []
    for how in ("device", "download"):
        ctx = api.Context(0)
        nrm = api.DeviceCloud(tgt, ctx=ctx).integral_normals_cloud()
        lib.check(L.rsreg_icp_set_target(ctx.h, t.ctypes.data, len(t), 32, 0, 0.05), ctx.h)
        if how == "device":
            lib.check(L.rsreg_icp_set_target_normals_cloud(ctx.h, nrm.h), ctx.h)
        else:
            rec = nrm.download_normals().points
            lib.check(L.rsreg_icp_set_target_normals(ctx.h, rec.ctypes.data, len(rec), 32), ctx.h)
        lib.check(L.rsreg_icp_set_source(ctx.h, s.ctypes.data, len(s), 32, 0), ctx.h)
        lib.check(L.rsreg_icp_begin(ctx.h, None, C.byref(prm)), ctx.h)
        lib.check(L.rsreg_icp_search(ctx.h, None, None), ctx.h)
        got = np.zeros(lib.NUM_PLANE_SUMS)
        lib.check(L.rsreg_icp_plane_sums(ctx.h, got.ctypes.data), ctx.h)
        lib.check(L.rsreg_icp_end(ctx.h, None, None, 0), ctx.h)
        sums.append(got)
    print("50k pair: pairs %d, with a normal %d" % (sums[0][0], sums[0][2]))
    assert sums[0].tobytes() == sums[1].tobytes()
    assert 1000 < sums[0][2] < sums[0][0] and np.isfinite(sums[0]).all()
