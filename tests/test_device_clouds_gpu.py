"""GPU: clouds that stay in HBM across the frame loop (rsreg_cloud_*, include/rsreg.h).  Every
device-resident step must hand back exactly the records its host-cloud counterpart does, and the
three schemes must produce the same merged clouds and transforms whether their frame loop runs
on host clouds (one upload + download per step) or on cloud handles (one upload per frame)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(rs):
    from rsreg_amd import api as a, lib
    lib.build()
    if a.device_count() < 1:
        pytest.fail("no HIP device: the product has no CPU fallback")
    return a


def _same_records(a, b):
    assert (len(a), a.width, a.height, a.is_dense) == (len(b), b.width, b.height, b.is_dense)
    for f in ("x", "y", "z", "w", "rgba"):
        np.testing.assert_array_equal(a.points[f].view(np.uint32), b.points[f].view(np.uint32))


@pytest.fixture(scope="module")
def frames(rs):
    out = [rs.synth.render_frame(k, "50k", "parity") for k in range(3)]
    out[1].points["x"][11] = np.nan          # a non-finite record travels through every step unchanged
    return out


def test_upload_download_copy_concat(api, rs, frames):
    a, b = frames[0], frames[1]
    da, db = api.DeviceCloud(a), api.DeviceCloud(b)
    assert len(da) == len(a) and da.info()[1:] == (32, a.width, a.height, a.is_dense) and isinstance(da.device_ptr, int) and da.device_ptr != 0
    _same_records(da.download(), a)
    _same_records(da.copy().download(), a)
    _same_records((da + db).download(), a + b)
    grown = da.copy()
    for _ in range(3):                      # repeated += : the buffer grows once, later appends copy only the new part
        grown.append(db)
    _same_records(grown.download(), a + b + b + b)
    empty = api.DeviceCloud(rs.PointCloud())
    assert len(empty) == 0 and len((empty + empty).download()) == 0
    _same_records((empty + da).download(), rs.PointCloud() + a)


@pytest.mark.parametrize("leaf", [(0.01, 0.01, 0.01), (1.0, 1.0, 1.0)])
def test_filter_and_transform_match_host_path(api, rs, frames, leaf):
    c = frames[1]
    ctx = api.default_context()
    vd, vh = api.ApproximateVoxelGrid(ctx), api.ApproximateVoxelGrid(ctx)
    vd.setLeafSize(*leaf)
    vh.setLeafSize(*leaf)
    vd.setInputCloud(api.DeviceCloud(c))
    vh.setInputCloud(c)
    _same_records(vd.filter().download(), vh.filter())
    T = rs.synth.small_transform(3.0, (0.01, -0.02, 0.03)).astype(np.float32)
    _same_records(api.transformPointCloud(api.DeviceCloud(c), T).download(), api.transformPointCloud(c, T))


def test_icp_and_ndt_on_handles_match_host_clouds(api, rs, frames):
    tgt, src = frames[0], frames[1]
    guess = rs.synth.small_transform(0.05, (0.001, 0.0, -0.0005)).astype(np.float32)
    for prm in (api.icp_params(reference=True), api.icp_params(max_iterations=6, criteria_mode=1, pipeline_mode=2, max_correspondence_distance=0.02)):
        out = []
        for dev in (False, True):
            icp = api.IterativeClosestPoint()
            icp.params = prm
            icp.setInputSource(api.DeviceCloud(src) if dev else src)
            icp.setInputTarget(api.DeviceCloud(tgt) if dev else tgt)
            aligned = icp.align(guess)
            out.append((aligned.download() if dev else aligned, bytes(icp.result.transform), icp.result.iterations, icp.result.n_correspondences))
        assert out[0][1:] == out[1][1:]
        _same_records(out[0][0], out[1][0])
    out = []
    for dev in (False, True):
        ndt = api.NormalDistributionsTransform()
        ndt.params = api.ndt_params(reference=True)
        ndt.setInputSource(api.DeviceCloud(src) if dev else src)
        ndt.setInputTarget(api.DeviceCloud(tgt) if dev else tgt)
        aligned = ndt.align(guess)
        out.append((aligned.download() if dev else aligned, bytes(ndt.result.transform), ndt.result.iterations, ndt.result.n_derivative_passes))
    assert out[0][1:] == out[1][1:]
    _same_records(out[0][0], out[1][0])


@pytest.mark.parametrize("kind", ["incremental", "icp_edge", "ndt_edge"])
def test_schemes_device_loop_equals_host_loop(api, rs, kind):
    from rsreg_amd import schemes
    frames = [rs.synth.render_frame(k, "50k", "bench") for k in range(3)]
    res = []
    # host clouds; cloud handles (the frame loop resident in HBM)
    for backend in (schemes.HipBackend(), schemes.HipDeviceBackend()):
        if kind == "incremental":
            s = schemes.IncrementalICP(backend=backend)
        else:
            cls = schemes.ICPEdgeBasedRegistration if kind == "icp_edge" else schemes.NDTEdgeBasedRegistration
            s = cls(rads=-0.0261799, backend=backend)
        clouds = [f.copy() for f in frames]
        merged = s.registration(clouds)
        tr = s.transforms if kind == "incremental" else [t for pair in s.frame_transforms for t in pair]
        res.append((merged, clouds[0], [np.asarray(t).tobytes() for t in tr]))
    (ma, c0a, ta) = res[0]
    for mb, c0b, tb in res[1:]:
        assert ta == tb and len(ta) >= 1
        _same_records(ma, mb)
        _same_records(c0a, c0b)                 # what the scheme did to the caller's frame 0 is the same too
        if kind == "incremental":
            assert ma is c0a and mb is c0b      # the reference returns (and grows) the caller's frame 0


def test_cloud_buffers_are_recycled_without_changing_results(api, rs, frames, monkeypatch):
    """Dropped clouds hand their buffers to the context's pool (no hipFree per drop).  A frame loop that creates and
    drops clouds of many sizes gives the same records with the pool (default), with a pool too small to keep anything,
    and with the pool switched off."""
    a, b = frames[0], frames[2]
    T = rs.synth.small_transform(2.0, (0.01, 0.02, -0.01)).astype(np.float32)

    def loop(ctx):
        out = []
        model = api.DeviceCloud(a, ctx)
        v = api.ApproximateVoxelGrid(ctx)
        v.setLeafSize(0.02, 0.02, 0.02)
        for k in range(6):
            f = api.DeviceCloud(b if k & 1 else a, ctx)
            v.setInputCloud(f)
            small = v.filter()                                  # a new, smaller cloud every round
            moved = api.transformPointCloud(f, T, ctx)
            moved = api.transformPointCloud(moved, T, ctx)      # the first `moved` is dropped: its buffer comes back below
            model = small + model                               # the old model is dropped, a larger one takes over
            model = model + moved
            out.append(small.download())
            del f, small, moved
        icp = api.IterativeClosestPoint(ctx)
        icp.params = api.icp_params(max_iterations=5, criteria_mode=1, max_correspondence_distance=0.05)
        icp.setInputSource(api.DeviceCloud(b, ctx))             # (buffers that have been through the pool)
        icp.setInputTarget(api.DeviceCloud(a, ctx))
        icp.align()
        out.append(model.download())
        return out, icp.getFinalTransformation().tobytes()

    ref, t_ref = loop(api.Context(0))
    for mb in ("0", "1"):
        monkeypatch.setenv("RSREG_CLOUD_POOL_MB", mb)
        got, t = loop(api.Context(0))
        assert t == t_ref
        for x, y in zip(ref, got):
            _same_records(x, y)


def test_upload_async_is_waited_for_by_every_consumer(api, rs, frames):
    """rsreg_cloud_upload_async returns with the PCIe copy still in flight; whatever touches the cloud next must see
    the uploaded records: download, copy, filter, transform, concatenation (either side), device pointer, an alignment
    (source and target), re-upload into the same handle, and a drop right after the call."""
    a, b = frames[0], frames[2]
    ctx = api.Context(0)
    T = rs.synth.small_transform(2.0, (0.01, 0.02, -0.01)).astype(np.float32)

    def fresh(c):
        return api.DeviceCloud(ctx=ctx).upload_async(c)

    _same_records(fresh(a).download(), a)
    _same_records(fresh(b).copy().download(), b)
    _same_records(api.transformPointCloud(fresh(a), T, ctx).download(), api.transformPointCloud(a, T, ctx))
    _same_records((fresh(a) + fresh(b)).download(), a + b)
    grown = fresh(a)
    grown.append(fresh(b))
    _same_records(grown.download(), a + b)
    v1, v2 = api.ApproximateVoxelGrid(ctx), api.ApproximateVoxelGrid(ctx)
    for v in (v1, v2):
        v.setLeafSize(0.02, 0.02, 0.02)
    v1.setInputCloud(fresh(b))
    v2.setInputCloud(b)
    _same_records(v1.filter().download(), v2.filter())
    c = fresh(a)
    assert isinstance(c.device_ptr, int) and c.device_ptr != 0
    assert c.info()[0] == len(a)
    again = fresh(a).upload_async(b)          # a second upload into a handle whose first is still in flight
    _same_records(again.download(), b)
    for _ in range(4):                         # more uploads in flight than staging buffers; some dropped at once
        fresh(a)
        keep = fresh(b)
    _same_records(keep.download(), b)
    res = []
    for src, tgt in ((fresh(b), fresh(a)), (api.DeviceCloud(b, ctx), api.DeviceCloud(a, ctx))):
        icp = api.IterativeClosestPoint(ctx)
        icp.params = api.icp_params(max_iterations=5, criteria_mode=1, max_correspondence_distance=0.05)
        icp.setInputSource(src)
        icp.setInputTarget(tgt)
        out = icp.align()
        res.append((icp.getFinalTransformation().tobytes(), out.download()))
    assert res[0][0] == res[1][0]
    _same_records(res[0][1], res[1][1])


def test_target_index_of_an_unchanged_cloud_can_be_kept(api, rs, frames):
    """rsreg_icp_target_is_cloud: 1 only for the very cloud the index was built from, unchanged, at the same gate.  A
    second ICP object that opts in (reuse_target_index) skips the build and gets the same bits; without the opt-in, or
    once the cloud has been rewritten in place, the index is built again."""
    from rsreg_amd import lib
    L = lib.lib()
    ctx = api.Context(0)
    tgt, src = api.DeviceCloud(frames[0], ctx), api.DeviceCloud(frames[2], ctx)
    other = api.DeviceCloud(frames[0], ctx)
    prm = dict(max_iterations=4, criteria_mode=1, max_correspondence_distance=0.05)

    def run(reuse):
        icp = api.IterativeClosestPoint(ctx)
        icp.params = api.icp_params(**prm)
        icp.reuse_target_index = reuse
        icp.setInputSource(src)
        icp.setInputTarget(tgt)
        icp.align()
        return icp.getFinalTransformation().tobytes(), icp.grid_info()

    t0, g0 = run(False)
    assert L.rsreg_icp_target_is_cloud(ctx.h, tgt.h, 0.05) == 1
    assert L.rsreg_icp_target_is_cloud(ctx.h, tgt.h, 0.01) == 0          # another gate: another index
    assert L.rsreg_icp_target_is_cloud(ctx.h, other.h, 0.05) == 0        # same records, another cloud
    t1, g1 = run(True)
    assert t1 == t0 and g1.n_cells == g0.n_cells
    tgt.append(other)                                                    # rewritten in place: same handle, new contents
    assert L.rsreg_icp_target_is_cloud(ctx.h, tgt.h, 0.05) == 0
    t2, g2 = run(True)
    assert g2.n_unique_points >= g0.n_unique_points
    fresh = api.IterativeClosestPoint(ctx)
    fresh.params = api.icp_params(**prm)
    fresh.setInputSource(src)
    fresh.setInputTarget(api.DeviceCloud(frames[0] + frames[0], ctx))
    fresh.align()
    assert fresh.getFinalTransformation().tobytes() == t2
    host = api.IterativeClosestPoint(ctx)                                # a target set another way forgets the cloud
    host.params = api.icp_params(**prm)
    host.setInputSource(frames[2])
    host.setInputTarget(frames[0])
    host.align()
    assert L.rsreg_icp_target_is_cloud(ctx.h, tgt.h, 0.05) == 0


@pytest.mark.parametrize("gate", [0.01, 0.05, 0.5, None])
def test_handful_of_queries_without_an_index(api, rs, frames, gate, monkeypatch):
    """With at most 64 source points (what IncrementalICP's 1 m voxel filter leaves of a frame) a device-cloud target is
    not indexed: every target point is scored against every query.  Matches (index and squared distance, bit for bit),
    iteration counts and transforms must be those of the indexed search; ties go to the lowest index; non-finite points
    on either side take no part; an alignment that turns out to need the index (more source points) gets it."""
    rng = np.random.default_rng(5)
    tgt = frames[0].copy()
    tgt.points[["x", "y", "z"]][100:110] = tgt.points[["x", "y", "z"]][50:60]        # value-equal copies: the lower index wins
    tgt.points["y"][7] = np.inf
    pick = rng.choice(len(frames[2]), 23, replace=False)
    few = rs.PointCloud(np.ascontiguousarray(frames[2].points[pick]))
    few.points[["x", "y", "z"]][3] = tgt.points[["x", "y", "z"]][55]                 # a query sitting on a duplicated target point
    few.points[["x", "y", "z"]][4] = few.points[["x", "y", "z"]][5]                  # two copies of one query
    few.points["z"][9] = np.nan
    kw = dict(max_iterations=6, criteria_mode=1)
    if gate is not None:
        kw["max_correspondence_distance"] = gate

    def run(no_scan, src):
        if no_scan:
            monkeypatch.setenv("RSREG_NO_SCAN", "1")
        else:
            monkeypatch.delenv("RSREG_NO_SCAN", raising=False)
        ctx = api.Context(0)
        icp = api.IterativeClosestPoint(ctx)
        icp.params = api.icp_params(**kw)
        icp.setInputSource(api.DeviceCloud(src, ctx))
        icp.setInputTarget(api.DeviceCloud(tgt, ctx))
        icp.begin()
        idx, d2 = icp.search()
        kind = icp.grid_info().index_kind
        out = icp.align()
        return kind, idx, d2, icp.getFinalTransformation().tobytes(), icp.result.iterations, icp.result.n_correspondences, out.download()

    a, b = run(False, few), run(True, few)
    assert a[0] == 2 and b[0] == 1
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert a[3:6] == b[3:6]
    _same_records(a[6], b[6])
    assert (a[1] >= 0).sum() >= (3 if gate == 0.01 else 10) and a[1][9] == -1
    if gate is None or gate >= 0.05:
        assert a[1][3] == 50 + 5                                                     # not its copy at 105
    many = rs.PointCloud(np.ascontiguousarray(frames[2].points[:5000]))
    c, d = run(False, many), run(True, many)
    assert c[0] == 1 and c[3:6] == d[3:6]
    # the target set for a handful of queries, then a larger source without setting the target again
    monkeypatch.delenv("RSREG_NO_SCAN", raising=False)
    ctx = api.Context(0)
    icp = api.IterativeClosestPoint(ctx)
    icp.params = api.icp_params(**kw)
    icp.setInputSource(api.DeviceCloud(few, ctx))
    keep = api.DeviceCloud(tgt, ctx)
    icp.setInputTarget(keep)
    icp.align()
    assert icp.grid_info().index_kind == 2 and icp.getFinalTransformation().tobytes() == b[3]
    icp.setInputSource(api.DeviceCloud(many, ctx))
    icp.align()
    assert icp.grid_info().index_kind == 1
    assert (icp.getFinalTransformation().tobytes(), icp.result.iterations, icp.result.n_correspondences) == d[3:6]


@pytest.mark.parametrize("leaf", [(1.0, 1.0, 1.0), (0.02, 0.02, 0.02)])
def test_filter_async_equals_filter(api, rs, frames, leaf):
    """rsreg_cloud_filter_async runs the filter on a side stream with scratch of its own and returns with the voxel sums
    still running: the records are those of the blocking filter, whatever touches the result first (download, an
    alignment as source or target, a transform), also with several filters issued back to back, with the main stream busy
    in between, and with inputs whose own upload was still in flight."""
    ctx = api.Context(0)
    a, b = frames[0], frames[2]
    T = rs.synth.small_transform(2.0, (0.01, 0.02, -0.01)).astype(np.float32)

    def vox():
        v = api.ApproximateVoxelGrid(ctx)
        v.setLeafSize(*leaf)
        return v

    def blocking(c):
        v = vox()
        v.setInputCloud(api.DeviceCloud(c, ctx))
        return v.filter().download()

    def side(c, in_flight=False):
        v = vox()
        v.setInputCloud(api.DeviceCloud(ctx=ctx).upload_async(c) if in_flight else api.DeviceCloud(c, ctx))
        return v.filter_async()

    ra, rb = blocking(a), blocking(b)
    _same_records(side(a).download(), ra)
    _same_records(side(b, in_flight=True).download(), rb)
    outs = [side(a), side(b), side(a, True), side(b, True)]          # back to back: one scratch set, in stream order
    big = api.DeviceCloud(a, ctx)
    for _ in range(3):
        big = big + big                                               # main stream busy meanwhile
    for o, r in zip(outs, (ra, rb, ra, rb)):
        _same_records(o.download(), r)
    _same_records(api.transformPointCloud(side(a), T, ctx).download(), api.transformPointCloud(ra, T, ctx))
    res = []
    for src in (side(b), api.DeviceCloud(rb, ctx)):
        icp = api.IterativeClosestPoint(ctx)
        icp.params = api.icp_params(max_iterations=5, criteria_mode=1, max_correspondence_distance=0.5)
        icp.setInputSource(src)
        icp.setInputTarget(api.DeviceCloud(a, ctx))
        icp.align()
        res.append((icp.getFinalTransformation().tobytes(), icp.result.n_correspondences))
    assert res[0] == res[1]


def test_device_cloud_rewritten_in_place_is_loaded_again(api, rs, frames):
    """PCL reads its inputs through pointers: a cloud rewritten in place between two align() calls is what the second
    one registers.  The wrappers compare (id, version) of a device cloud with what they loaded (rsreg_cloud_version)
    and load it again; the C ABI itself refuses to write an aligned cloud from a source handle that has changed or
    gone since rsreg_icp_set_source_cloud (RSREG_ERR_STATE) instead of touching freed memory."""
    import ctypes as C

    from rsreg_amd import lib
    L = lib.lib()
    ctx = api.Context(0)
    prm = dict(max_iterations=3, criteria_mode=1, max_correspondence_distance=0.05)
    tgt, src = api.DeviceCloud(frames[0], ctx), api.DeviceCloud(frames[2], ctx)
    icp = api.IterativeClosestPoint(ctx)
    icp.params = api.icp_params(**prm)
    icp.setInputSource(src)
    icp.setInputTarget(tgt)
    icp.align()
    s0 = src.stamp
    assert src.stamp == s0 and tgt.stamp[0] != s0[0]
    tgt.append(api.DeviceCloud(frames[1], ctx))          # target grown in place, setInputTarget not called again
    T = rs.synth.small_transform(0.4, (0.002, 0.001, -0.003)).astype(np.float32)
    _check = lib.check
    _check(L.rsreg_cloud_transform(ctx.h, src.h, np.ascontiguousarray(T.T).ctypes.data, src.h), ctx.h)   # source moved in place
    assert src.stamp == (s0[0], s0[1] + 1)
    icp.align()
    fresh = api.IterativeClosestPoint(api.Context(0))
    fresh.params = api.icp_params(**prm)
    fresh.setInputSource(api.transformPointCloud(frames[2], T))
    fresh.setInputTarget(frames[0] + frames[1])
    fresh.align()
    assert icp.getFinalTransformation().tobytes() == fresh.getFinalTransformation().tobytes()
    ndt = api.NormalDistributionsTransform(ctx)
    ndt.setInputSource(src)
    ndt.setInputTarget(tgt)
    ndt.align()
    n0 = ndt.result.n_voxels
    tgt.append(api.DeviceCloud(api.transformPointCloud(frames[1], rs.synth.small_transform(0.0, (0.0, 3.0, 0.0)).astype(np.float32)), ctx))
    ndt.align()                                           # the voxel grid is rebuilt from the grown cloud
    assert ndt.result.n_voxels > n0

    # C ABI: the source handle is destroyed (or rewritten) before the aligned cloud is asked for
    gone = api.DeviceCloud(frames[2], ctx)
    out = api.DeviceCloud(ctx=ctx)
    res, p = lib.IcpResult(), api.icp_params(**prm)
    _check(L.rsreg_icp_set_source_cloud(ctx.h, gone.h), ctx.h)
    _check(L.rsreg_icp_set_target_cloud(ctx.h, tgt.h, 0.05), ctx.h)
    gone.close()
    assert L.rsreg_icp_align_cloud(ctx.h, None, C.byref(p), C.byref(res), out.h) == lib.RSREG_ERR_STATE
    assert L.rsreg_icp_align_cloud(ctx.h, None, C.byref(p), C.byref(res), None) == 0      # the 4x4 alone needs no handle
    again = api.DeviceCloud(frames[2], ctx)
    _check(L.rsreg_icp_set_source_cloud(ctx.h, again.h), ctx.h)
    again.upload(frames[1])
    assert L.rsreg_icp_align_cloud(ctx.h, None, C.byref(p), C.byref(res), out.h) == lib.RSREG_ERR_STATE
    # edge extraction checks that both handles belong to the context it is called on
    other_ctx = api.Context(0)
    organized = api.DeviceCloud(rs.synth.render_frame(0, (64, 48), "parity"), ctx)
    assert L.rsreg_cloud_edge_features(other_ctx.h, organized.h, out.h) == lib.RSREG_ERR_INVALID_ARG


def test_grown_target_is_indexed_as_it_is_now(api, rs, frames):
    """The edge-based schemes put every frame's refined points in FRONT of the target they were aligned with and set
    the grown cloud as the next target (icp_edge_based_registration.hpp:79,109,119-120); PCL builds a new kd-tree each
    time.  A cloud handle that has grown -- in front, behind, by points outside the old box, by exact copies -- must be
    searched as the cloud it is now: matches and transforms those of a fresh context given the same records on the host.
    (Rounds 3-4 merged the new records into the old index instead; it was bit-identical and did not pay,
    profiles/r04_experiments/README.md: the index is built afresh.)"""
    ctx = api.Context(0)
    prm = dict(max_iterations=3, criteria_mode=1, max_correspondence_distance=0.05)
    src = frames[2]

    def search(icp):
        icp.begin()
        idx, d2 = icp.search()
        icp.end()
        return idx, d2

    def fresh(host_target):
        f = api.IterativeClosestPoint(api.Context(0))
        f.params = api.icp_params(**prm)
        f.setInputSource(src)
        f.setInputTarget(host_target)
        i, d = search(f)
        f.align()
        return i, d, f.getFinalTransformation().tobytes(), f.grid_info()

    tgt = api.DeviceCloud(frames[0], ctx)
    icp = api.IterativeClosestPoint(ctx)
    icp.params = api.icp_params(**prm)
    icp.setInputSource(api.DeviceCloud(src, ctx))
    icp.setInputTarget(tgt)
    icp.align()
    host = frames[0]

    def valid(c):
        pts = np.ascontiguousarray(c.points[np.isfinite(c.points["x"]) & (c.points["z"] != 0)])
        return rs.PointCloud(pts, width=len(pts), height=1, is_dense=False)

    far = api.transformPointCloud(valid(frames[1].crop(0, 0, 100, 40)), rs.synth.small_transform(0.0, (7.0, 0.0, 0.0)).astype(np.float32))
    steps = [("front", api.transformPointCloud(valid(frames[1].crop(0, 0, 250, 60)), rs.synth.small_transform(0.3, (0.004, 0.0, -0.003)).astype(np.float32))),
             ("back", api.transformPointCloud(valid(frames[1].crop(0, 100, 250, 50)), rs.synth.small_transform(-0.2, (0.0, 0.002, 0.001)).astype(np.float32))),
             ("front", far), ("front", frames[0].crop(10, 10, 50, 50)), ("back", frames[1])]
    for where, new in steps:
        d_new = api.DeviceCloud(new, ctx)
        if where == "front":
            tgt.prepend(d_new)
            host = new + host
        else:
            tgt.append(d_new)
            host = host + new
        icp.setInputTarget(tgt)
        i1, d1 = search(icp)
        icp.align()
        g = icp.grid_info()
        i0, d0, t0, g0 = fresh(host)
        np.testing.assert_array_equal(i1, i0)
        np.testing.assert_array_equal(d1, d0)
        assert icp.getFinalTransformation().tobytes() == t0
        assert (g.n_unique_points, g.n_target_points, g.n_cells) == (g0.n_unique_points, g0.n_target_points, g0.n_cells)
    # a cloud rewritten in place (a transform) is indexed again too
    tgt2 = api.DeviceCloud(frames[0], ctx)
    icp.setInputTarget(tgt2)
    icp.align()
    api._l.check(api._l.lib().rsreg_cloud_transform(ctx.h, tgt2.h, api._colmajor(rs.synth.small_transform(0.2, (0.01, 0.0, 0.0)).astype(np.float32)).ctypes.data,
                                                    tgt2.h), ctx.h)
    icp.setInputTarget(tgt2)
    i1, d1 = search(icp)
    moved = api.transformPointCloud(frames[0], rs.synth.small_transform(0.2, (0.01, 0.0, 0.0)).astype(np.float32))
    i0, d0, _, _ = fresh(moved)
    np.testing.assert_array_equal(i1, i0)
    np.testing.assert_array_equal(d1, d0)


def test_download_async_lands_what_the_stream_had_when_it_was_asked(api, rs, frames):
    """rsreg_cloud_download_async returns at once; the host array holds the records the cloud had at the point of the
    call once rsreg_ctx_wait_downloads has returned, whatever happened to the cloud right after: rewritten by an
    upload, a transform INTO it, an append, or dropped.  More downloads in flight than the context has staging slots;
    an empty cloud; a second wait is a no-op; the bad calls are refused."""
    a, b, c = frames
    ctx = api.Context(0)
    T = rs.synth.small_transform(2.0, (0.01, 0.02, -0.01)).astype(np.float32)
    na, nb, nc = len(a), len(b), len(c)
    moved_b = api.transformPointCloud(b, T, ctx)
    out = np.zeros(na * 3 + nb * 3 + nc + 7, api.POINT_DTYPE)
    out["rgba"] = 0xDEADBEEF
    at, want = 0, []

    def push(dc, expect):
        nonlocal at
        got = dc.download_async(out, at)
        assert got == len(expect)
        want.append((at, expect))
        at += got

    da = api.DeviceCloud(a, ctx)
    push(da, a)
    da.upload(b)                               # rewritten at once: the copy in flight is of `a`
    push(da, b)
    db = api.DeviceCloud(ctx=ctx).upload_async(b)   # an upload still in flight behind it
    push(db, b)
    moved = api.transformPointCloud(db, T, ctx)
    push(moved, moved_b)
    del moved                                  # dropped with its download in flight
    grown = api.DeviceCloud(a, ctx)
    push(grown, a)
    grown.append(api.DeviceCloud(c, ctx))      # grows (and may move) the buffer right after
    push(api.DeviceCloud(c, ctx), c)           # a temporary
    push(api.DeviceCloud(rs.PointCloud(), ctx), rs.PointCloud())
    push(api.DeviceCloud(a, ctx), a)
    ctx.wait_downloads()
    ctx.wait_downloads()
    for lo, expect in want:
        for f in ("x", "y", "z", "w", "rgba"):
            np.testing.assert_array_equal(out[f][lo:lo + len(expect)].view(np.uint32), expect.points[f].view(np.uint32))
    assert at == na * 3 + nb * 3 + nc and (out["rgba"][at:] == 0xDEADBEEF).all()   # nothing written past the records
    _same_records(grown.download(), a + c)
    with pytest.raises(ValueError):
        da.download_async(out, len(out) - 1)
    with pytest.raises(ValueError):
        da.download_async(np.zeros(nb, np.float32))
    small = np.zeros(3, api.POINT_DTYPE)
    from rsreg_amd import lib
    assert lib.lib().rsreg_cloud_download_async(da.h, small.ctypes.data, 3) == lib.RSREG_ERR_INVALID_ARG
    assert lib.lib().rsreg_cloud_download_async(None, small.ctypes.data, 3) != 0
    assert lib.lib().rsreg_ctx_wait_downloads(None) != 0


def test_upload_deferred_is_waited_for_like_upload_async(api, rs, frames):
    """rsreg_cloud_upload_deferred returns before the records have been read (a thread of the context stages them);
    every consumer still sees them: download, copy, transform, an alignment, a second deferred upload into the same
    handle, more uploads in flight than staging buffers, a drop right after the call, and deferred and async uploads
    mixed on one context."""
    a, b, c = frames
    ctx = api.Context(0)
    T = rs.synth.small_transform(2.0, (0.01, 0.02, -0.01)).astype(np.float32)

    def later(cl):
        return api.DeviceCloud(ctx=ctx).upload_deferred(cl)

    _same_records(later(a).download(), a)
    _same_records(later(b).copy().download(), b)
    _same_records(api.transformPointCloud(later(a), T, ctx).download(), api.transformPointCloud(a, T, ctx))
    again = later(a).upload_deferred(b)
    _same_records(again.download(), b)
    held = [later(x) for x in (a, b, c, a, b, c)]          # six in flight, two staging buffers
    mixed = api.DeviceCloud(ctx=ctx).upload_async(c)
    later(a)                                               # dropped at once
    for dc, want in zip(held, (a, b, c, a, b, c)):
        _same_records(dc.download(), want)
    _same_records(mixed.download(), c)
    _same_records((later(a) + later(b)).download(), a + b)
    res = []
    for src, tgt in ((later(b), later(a)), (api.DeviceCloud(b, ctx), api.DeviceCloud(a, ctx))):
        icp = api.IterativeClosestPoint(ctx)
        icp.params = api.icp_params(max_iterations=5, criteria_mode=1, max_correspondence_distance=0.05)
        icp.setInputSource(src)
        icp.setInputTarget(tgt)
        out = icp.align()
        res.append((icp.getFinalTransformation().tobytes(), out.download()))
    assert res[0][0] == res[1][0]
    _same_records(res[0][1], res[1][1])
    empty = later(rs.PointCloud())
    assert len(empty) == 0 and len(empty.download()) == 0
    from rsreg_amd import lib
    assert lib.lib().rsreg_cloud_upload_deferred(None, None, 0, 32, 0, 0, 1) == lib.RSREG_ERR_INVALID_ARG
    assert lib.lib().rsreg_cloud_upload_deferred(held[0].h, None, 5, 32, 5, 1, 1) == lib.RSREG_ERR_INVALID_ARG


def test_edge_features_and_filter_queued_on_the_side_worker(api, rs):
    """rsreg_cloud_edge_features_async and rsreg_cloud_filter_async return before their jobs have run; the results have
    the records of the synchronous calls once anything asks for them: a frame still uploading as the input, the filter
    chained on the not-yet-run extraction, several frames in flight over the three scratch sets, results dropped unread,
    a frame without a single edge, the size asked for first (info), and the bad calls refused."""
    ctx = api.Context(0)
    frames = [rs.synth.render_frame(k, "50k", "bench") for k in range(5)]
    leaf = np.array([0.01, 0.01, 0.01], np.float32)

    def sync_chain(f):
        e = api.extract_edge_features(api.DeviceCloud(f, ctx))
        v = api.ApproximateVoxelGrid(ctx)
        v.setLeafSize(*leaf)
        v.setInputCloud(e)
        return e.download(), v.filter().download()

    want = [sync_chain(f) for f in frames]
    queued = []
    for f in frames:                               # five frames, three scratch sets: the jobs take turns
        d = api.DeviceCloud(ctx=ctx).upload_deferred(f)
        e = api.extract_edge_features_async(d)
        v = api.ApproximateVoxelGrid(ctx)
        v.setLeafSize(*leaf)
        v.setInputCloud(e)
        queued.append((e, v.filter_async()))
    for (e, r), (we, wr) in zip(reversed(queued), reversed(want)):     # asked for in another order than posted
        assert r.info()[0] == len(wr)
        _same_records(r.download(), wr)
        _same_records(e.download(), we)
    # dropped unread, with the jobs possibly still queued
    d = api.DeviceCloud(ctx=ctx).upload_deferred(frames[0])
    e = api.extract_edge_features_async(d)
    v = api.ApproximateVoxelGrid(ctx)
    v.setLeafSize(*leaf)
    v.setInputCloud(e)
    r = v.filter_async()
    del r, e, d
    # no edge anywhere: both results empty
    flat = frames[0].copy()
    flat.points["rgba"] = 0x00808080
    e = api.extract_edge_features_async(api.DeviceCloud(flat, ctx))
    v.setInputCloud(e)
    r = v.filter_async()
    assert len(r) == 0 and len(e) == 0 and len(r.download()) == 0
    # a result feeds the synchronous calls like any other cloud
    e = api.extract_edge_features_async(api.DeviceCloud(frames[1], ctx))
    v.setInputCloud(e)
    _same_records(v.filter().download(), want[1][1])
    from rsreg_amd import lib
    L = lib.lib()
    unorganized = api.DeviceCloud(frames[0] + frames[1], ctx)      # (one row of 2 n points: still an image, like the synchronous call takes it)
    out = api.DeviceCloud(ctx=ctx)
    assert L.rsreg_cloud_edge_features_async(ctx.h, out.h, out.h) == lib.RSREG_ERR_INVALID_ARG
    assert L.rsreg_cloud_edge_features_async(ctx.h, None, out.h) == lib.RSREG_ERR_INVALID_ARG
    other = api.Context(0)
    assert L.rsreg_cloud_edge_features_async(other.h, unorganized.h, out.h) == lib.RSREG_ERR_INVALID_ARG


def test_side_jobs_on_two_workers_give_the_synchronous_results(api, rs):
    """Round 6: the side jobs of a context alternate between two worker threads (two scratch sets and streams each); a job
    whose input is the output of a job still queued follows it on the same worker.  Twelve frames' extractions, each with
    two filters chained on it (one more than a worker has sets), all queued before anything is asked for: the records of
    the synchronous calls, on the two workers."""
    ctx = api.Context(0)
    frames = [rs.synth.render_frame(k, "50k", "bench") for k in range(12)]
    leaves = (np.array([0.01, 0.01, 0.01], np.float32), np.array([0.05, 0.04, 0.03], np.float32))

    def filt(cloud, leaf, queued):
        v = api.ApproximateVoxelGrid(ctx)
        v.setLeafSize(*leaf)
        v.setInputCloud(cloud)
        return v.filter_async() if queued else v.filter()

    want = []
    for f in frames:
        e = api.extract_edge_features(api.DeviceCloud(f, ctx))
        want.append((e.download(), filt(e, leaves[0], False).download(), filt(e, leaves[1], False).download()))
    queued = []
    for f in frames:
        d = api.DeviceCloud(ctx=ctx).upload_deferred(f)
        e = api.extract_edge_features_async(d)
        queued.append((d, e, filt(e, leaves[0], True), filt(e, leaves[1], True)))
    for k in (5, 0, 11, 3, 8, 1, 10, 2, 9, 4, 7, 6):
        _, e, r0, r1 = queued[k]
        _same_records(r1.download(), want[k][2])
        _same_records(e.download(), want[k][0])
        _same_records(r0.download(), want[k][1])


def test_contexts_and_clouds_go_away_with_work_of_their_helper_threads_in_flight(api, rs):
    """A context owns helper threads (uploads, downloads, side jobs, source loads).  Dropping clouds, and closing the
    context, right after work has been handed to them must neither hang nor crash, whatever is still queued; a context
    made afterwards works as usual."""
    frames = [rs.synth.render_frame(k, "50k", "bench") for k in range(3)]
    for round_ in range(3):
        ctx = api.Context(0)
        out = np.zeros(sum(len(f) for f in frames), api.POINT_DTYPE)
        clouds, at = [], 0
        for f in frames:
            d = api.DeviceCloud(ctx=ctx).upload_deferred(f)
            e = api.extract_edge_features_async(d)
            v = api.ApproximateVoxelGrid(ctx)
            v.setLeafSize(0.01, 0.01, 0.01)
            v.setInputCloud(e)
            r = v.filter_async()
            at += api.DeviceCloud(f, ctx).download_async(out, at)
            clouds.append((d, e, r))
        if round_ == 0:
            del clouds                       # outputs first or inputs first: whatever the collector does
        elif round_ == 1:
            clouds.reverse()
            while clouds:
                clouds.pop()
        ctx.wait_downloads() if round_ == 2 else None
        ctx.close()                          # (round 2: with the clouds still alive; they are not touched again)
        if round_ == 2:
            for f, lo in zip(frames, np.cumsum([0] + [len(f) for f in frames[:-1]])):
                np.testing.assert_array_equal(out["rgba"][lo:lo + len(f)], f.points["rgba"])
    ctx = api.Context(0)
    _same_records(api.DeviceCloud(frames[0], ctx).download(), frames[0])


def test_a_clouds_bounding_box_is_measured_once_per_version(api, rs):
    """A frame that was one pair's source is the next pair's target: its handle keeps the bounding box and the finite
    count the source load measured, and the index build starts from them instead of measuring again (one kernel pair and a
    round trip to the host less) -- for exactly the records that were measured: a handle rewritten since is measured anew."""
    from rsreg_amd import lib
    f = [rs.synth.render_frame(k, "N300", "parity") for k in range(3)]      # (> 65 536 points: the source load that sorts, and measures)
    f[1].points["y"][5] = np.inf
    prm = dict(max_iterations=2, criteria_mode=1, max_correspondence_distance=0.05)

    def pair(ctx, s, t):
        icp = api.IterativeClosestPoint(ctx)
        icp.params = api.icp_params(**prm)
        icp.setInputSource(s)
        icp.setInputTarget(t)
        icp.align()
        gi = icp.grid_info()
        return (icp.getFinalTransformation().tobytes(), tuple(gi.origin), tuple(gi.dims), gi.n_cells, gi.n_unique_points, gi.n_target_points,
                icp.result.n_correspondences)

    def fresh(s, t):
        c = api.Context(0)
        return pair(c, api.DeviceCloud(s, c), api.DeviceCloud(t, c))

    ctx = api.Context(0)
    dev = [api.DeviceCloud(x, ctx) for x in f]
    pair(ctx, dev[1], dev[0])                                # frame 1 is measured as a source ...
    assert pair(ctx, dev[2], dev[1]) == fresh(f[2], f[1])    # ... and indexed as a target from what its handle kept
    assert pair(ctx, dev[2], dev[1]) == pair(api.Context(0), f[2], f[1])   # (host clouds: measured inside the call, every time)
    assert pair(ctx, dev[2], dev[1]) == fresh(f[2], f[1])    # (both boxes kept now)
    moved = api.transformPointCloud(f[0], rs.synth.small_transform(0.0, (0.5, -0.25, 0.125)).astype(np.float32))
    dev[1].upload(moved)                                     # other records under the same handle: another box
    assert pair(ctx, dev[2], dev[1]) == fresh(f[2], moved)
    T = rs.synth.small_transform(0.0, (0.0, 1.0, 0.0)).astype(np.float32)
    lib.check(lib.lib().rsreg_cloud_transform(ctx.h, dev[2].h, np.ascontiguousarray(T.T).ctypes.data, dev[2].h), ctx.h)   # the source moved in place
    assert pair(ctx, dev[2], dev[1]) == fresh(api.transformPointCloud(f[2], T), moved)
    assert pair(ctx, dev[1], dev[2]) == fresh(moved, api.transformPointCloud(f[2], T))   # and the two the other way round
