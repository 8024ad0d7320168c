"""The plane segmentation on the GPU (csrc/segment.hip, csrc/plane_seg_kernels.hpp) against the numpy reference of
tests/plane_seg_ref.py: counts, hypotheses, whole segmentations and the two filters, for equality.  What each case is FOR is
asserted on the reference in tests/test_plane_seg_cpu.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import cluster_cases as CK
import layout_cases as LC
import plane_seg_cases as K
import plane_seg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QNAN = 0x7fc00000
CANARY = 0xA5A5A5A5
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


def _rec(points, sel):
    """the bytes of the selected records, padding included (indexing a structured array would leave the padding behind)"""
    return np.ascontiguousarray(points).view(np.uint8).reshape(len(points), -1)[sel].tobytes()


def _cloud(xyz):
    return CK.cloud(np.ascontiguousarray(xyz, np.float32).reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def _case(name):
    make, prm = K.SEGMENT_CASES[name]
    xyz = make()
    xyz.setflags(write=False)
    return xyz, prm


_REFS = {}


def _ref(api, name):
    if name not in _REFS:
        xyz, prm = _case(name)
        _REFS[name] = R.segment(api, xyz, **prm)
    return _REFS[name]


# ------------------------------------------------------------------------------------------------ plane_count
@pytest.mark.parametrize("n", K.COUNT_N)
def test_plane_count_equals_the_reference(api, ctx, n):
    xyz = K.count_cloud(n)
    dc = api.DeviceCloud(_cloud(xyz), ctx=ctx)
    for H in K.COUNT_H:
        models = K.count_models(H)
        for thr in (0.05, 0.0):
            got = dc.plane_count(models, thr) if H else dc.plane_count(np.zeros((0, 4), np.float32), thr)
            want = R.count(models, xyz, thr)
            assert got.dtype == np.uint32 and len(got) == H and (got == want).all(), (n, H, thr, np.flatnonzero(got != want)[:8])
        if H >= 12 and n >= K.TILE - 1:
            assert want.max() == 0 and R.count(models, xyz, 0.05)[11:].min() > 0


@pytest.mark.parametrize("stride", K.COUNT_STRIDES)
def test_plane_count_reads_every_record_layout(api, ctx, stride):
    xyz, models = K.count_cloud(K.TILE + 77), K.count_models(65)
    dc = api.DeviceCloud(LC.raw_cloud(xyz, stride), ctx=ctx)
    assert dc.info()[1] == stride and (dc.plane_count(models, 0.05) == R.count(models, xyz, 0.05)).all()


def test_plane_count_past_the_group_limit(api, ctx):
    """(tiles) x (chunks) passes kPlaneMaxGroups: a slice takes two chunks, and the last slice is ragged"""
    n, H = K.TILE + 5, K.MAX_GROUPS * K.CHUNK // 2 + 7
    tiles, chunks, per, slices = K.plan(n, H)
    assert tiles == 2 and per == 2 and tiles * chunks > K.MAX_GROUPS and chunks % per == 1
    xyz = K.count_cloud(n)
    models = K.count_models(200)[np.arange(H) % 200]
    models[:, 3] += (np.arange(H) // 200).astype(np.float32) * np.float32(0.003)
    got = api.DeviceCloud(_cloud(xyz), ctx=ctx).plane_count(models, 0.05)
    assert (got == R.count(models, xyz, 0.05, chunk=1024)).all()


@pytest.mark.parametrize("t", [np.float32(0.01), 0.01, 0.0625, 1e-3, 0.3])
def test_the_threshold_is_strict(api, ctx, t):
    """records at z = (float)t, one float below and one above, on both sides of the plane z = 0: inside iff (double)|z| < t"""
    xyz = K.threshold_records(t)
    got = api.DeviceCloud(_cloud(xyz), ctx=ctx)
    want = np.abs(xyz[:, 2]).astype(np.float64) < float(t)
    assert want[:8].all() and not want[16:].any()
    assert got.plane_count([0, 0, 1, 0], float(t))[0] == want.sum()
    out, kept = got.plane_filter([0, 0, 1, 0], float(t))
    assert kept == want.sum() and (out.download().xyz == xyz[want]).all()
    from rsreg_amd import lib
    for bad in (-0.01, float("nan")):
        with pytest.raises(lib.RsregError):
            got.plane_count([0, 0, 1, 0], bad)


# ------------------------------------------------------------------------------------------------ plane_hypotheses
@pytest.mark.parametrize("name", sorted(K.HYPOTHESIS_CASES))
def test_hypotheses_equal_the_reference(api, ctx, name):
    make, prm = K.HYPOTHESIS_CASES[name]
    xyz = make()
    want = R.hypotheses(xyz, prm["seed"], 0, K.HYPOTHESES, prm.get("axis", (0, 0, 0)), prm.get("eps_angle", 0.0))
    if "axis" in prm:
        assert min(abs(c - np.cos(prm["eps_angle"])) for c in want[3] if c is not None) > 1e-12
    dc = api.DeviceCloud(_cloud(xyz), ctx=ctx)
    coeffs, samples, valid = dc.plane_hypotheses(0, K.HYPOTHESES, **prm)
    assert (samples == want[1]).all(), np.flatnonzero((samples != want[1]).any(axis=1))[:8]
    assert (valid == want[2]).all()
    assert coeffs.view(np.uint32).tobytes() == want[0].view(np.uint32).tobytes(), np.flatnonzero((coeffs.view(np.uint32) != want[0].view(np.uint32)).any(axis=1))[:8]
    assert (coeffs.view(np.uint32)[~valid] == QNAN).all()
    # h_first > 0 gives the same rows as a larger call from 0
    c2, s2, v2 = dc.plane_hypotheses(137, 40, **prm)
    assert c2.tobytes() == coeffs[137:177].tobytes() and (s2 == samples[137:177]).all() and (v2 == valid[137:177]).all()


# ------------------------------------------------------------------------------------------------ plane_segment
def _check_segment(got, ref, name):
    coeff, inliers, res = got
    print("plane segment %s: found %d, hypothesis %d, iterations %d, skipped %d, inliers %d, refined %d" %
          (name, res.found, res.best_hypothesis, res.iterations, res.skipped, res.n_inliers, res.refined))
    assert (res.found, res.best_hypothesis, res.sample, res.iterations, res.skipped) == (ref.found, ref.best_hypothesis, ref.sample, ref.iterations, ref.skipped)
    assert res.unrefined.tobytes() == ref.unrefined.tobytes()
    assert res.sums.tobytes() == ref.sums.tobytes(), (res.sums, ref.sums)
    assert res.refined == ref.refined and coeff.tobytes() == np.asarray(ref.coeff, np.float32).tobytes()
    assert res.n_inliers == ref.n_inliers == len(inliers) and inliers.dtype == np.int32 and (inliers == ref.inliers).all()
    assert res.cos_eps == ref.cos_eps


@pytest.mark.parametrize("name", sorted(K.SEGMENT_CASES))
def test_segment_equals_the_reference(api, ctx, name):
    xyz, prm = _case(name)
    ref = _ref(api, name)
    if "axis" in prm:
        assert ref.min_cs_margin > 1e-12
    _check_segment(api.DeviceCloud(_cloud(xyz), ctx=ctx).segment_plane(**prm), ref, name)


def test_segment_capacity_and_nullable_outputs(api, ctx):
    from rsreg_amd import lib
    L = lib.lib()
    xyz, prm = _case("a60_s0")
    ref = _ref(api, "a60_s0")
    dc = api.DeviceCloud(_cloud(xyz), ctx=ctx)
    coeff, inliers, res = dc.segment_plane(capacity=100, **prm)
    assert res.n_inliers == ref.n_inliers > 100 and len(inliers) == 100 and (inliers == ref.inliers[:100]).all()
    p = api.plane_params(**prm)
    idx = np.full(ref.n_inliers + 5, CANARY, np.uint32)
    found = C.c_size_t(0)
    lib.check(L.rsreg_cloud_plane_segment(ctx.h, dc.h, C.byref(p), None, idx.ctypes.data, 7, C.byref(found), None), ctx.h)
    assert found.value == ref.n_inliers and (idx[:7].view(np.int32) == ref.inliers[:7]).all() and (idx[7:] == CANARY).all()
    lib.check(L.rsreg_cloud_plane_segment(ctx.h, dc.h, C.byref(p), None, None, 0, None, None), ctx.h)          # every output NULL
    assert L.rsreg_cloud_plane_segment(ctx.h, dc.h, C.byref(p), None, None, 5, C.byref(found), None) == lib.RSREG_ERR_INVALID_ARG
    for bad in (dict(probability=0.0), dict(probability=1.0), dict(max_iterations=-1), dict(eps_angle=-0.1), dict(eps_angle=float("nan")),
                dict(axis=(0.0, float("inf"), 1.0)), dict(distance_threshold=-1.0), dict(distance_threshold=float("nan"))):
        with pytest.raises(lib.RsregError) as e:
            dc.segment_plane(**dict(prm, **bad))
        assert e.value.status == lib.RSREG_ERR_INVALID_ARG
    assert L.rsreg_version() == 4


@pytest.mark.parametrize("name", ["a60_s0", "b_axis_z"])
def test_same_bytes_from_a_second_context(api, ctx, name):
    xyz, prm = _case(name)
    a = api.DeviceCloud(_cloud(xyz), ctx=ctx).segment_plane(**prm)
    other = api.Context(0)
    api.DeviceCloud(_cloud(K.count_cloud(700)), ctx=other).plane_count(K.count_models(65), 0.05)      # the fresh context has scored another cloud first
    b = api.DeviceCloud(_cloud(xyz), ctx=other).segment_plane(**prm)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for k in ("found", "best_hypothesis", "sample", "iterations", "skipped", "refined", "n_inliers", "cos_eps"):
        assert getattr(a[2], k) == getattr(b[2], k), k
    assert a[2].sums.tobytes() == b[2].sums.tobytes() and a[2].unrefined.tobytes() == b[2].unrefined.tobytes()
    _check_segment(b, _ref(api, name), name)


def test_two_rounds_on_scene_b_wall_then_floor(api, ctx):
    xyz, label = K.scene_b(0)
    dc = api.DeviceCloud(_cloud(xyz), ctx=ctx)
    c1, in1, r1 = dc.segment_plane(distance_threshold=K.THRESHOLD)
    assert r1.found and abs(c1[0]) > 0.99 and (label[in1] == 0).mean() > 0.95
    rest, kept = dc.plane_filter(c1, K.THRESHOLD, negative=True)
    keep = np.ones(len(xyz), bool)
    keep[in1] = False
    assert kept == keep.sum() == len(xyz) - r1.n_inliers and (rest.download().xyz == xyz[keep]).all()
    c2, in2, r2 = rest.segment_plane(distance_threshold=K.THRESHOLD)
    ref2 = R.segment(api, xyz[keep], distance_threshold=K.THRESHOLD)
    _check_segment((c2, in2, r2), ref2, "scene B, second round")
    assert r2.found and abs(c2[2]) > 0.99 and (label[keep][in2] == 1).mean() > 0.9 and r2.n_inliers > 550


def test_floor_removal_before_clustering(api, ctx):
    xyz, label = K.blobs_on_floor()
    dc = api.DeviceCloud(_cloud(xyz), ctx=ctx)
    with_floor = dc.euclidean_clusters(0.05, min_size=20)
    assert len(with_floor[2]) - 1 == 1                                             # the floor joins everything
    coeff, inliers, res = dc.segment_plane(distance_threshold=0.01)
    assert res.found and abs(coeff[2]) > 0.999 and (label[inliers] == -1).all() and res.n_inliers > 0.99 * (label == -1).sum()
    rest, kept = dc.plane_filter(coeff, 0.01, negative=True)
    labels, indices, offsets = rest.euclidean_clusters(0.05, min_size=20)
    assert len(offsets) - 1 == 3 and np.diff(offsets).tolist() == [150, 150, 150]
    left = label[np.setdiff1d(np.arange(len(xyz)), inliers)]
    for c in range(3):
        assert len(set(left[indices[offsets[c]:offsets[c + 1]]].tolist())) == 1   # every cluster is one blob


# ------------------------------------------------------------------------------------------------ plane_filter, extract_indices
def _download_words(out, stride, ctx):
    from rsreg_amd import lib
    n, got_stride = out.info()[:2]
    assert got_stride == stride or n == 0
    buf = np.zeros((n, stride // 4), np.uint32)
    lib.check(lib.lib().rsreg_cloud_download(out.h, buf.ctypes.data, n), ctx.h)
    return buf


@pytest.mark.parametrize("stride", [12, 16, 32, 48])
def test_filters_on_every_record_layout(api, ctx, stride):
    xyz = LC.non_finite_xyz()
    src = LC.words(xyz, stride)
    model, thr = np.array([0.6, 0.0, 0.8, -0.1], np.float32), 0.2
    inl = R.within(model, xyz, thr)[0]
    assert 100 < inl.sum() < len(xyz) - 400 and (~np.isfinite(xyz).all(axis=1)).sum() > 100
    dc = api.DeviceCloud(LC.raw_cloud(xyz, stride, 60, 50), ctx=ctx)
    for negative in (False, True):
        keep = inl != negative
        out, kept = dc.plane_filter(model, thr, negative=negative)
        assert kept == keep.sum() and _download_words(out, stride, ctx).tobytes() == src[keep].tobytes()     # bytes beyond xyz carried unchanged
        assert out.info()[2:4] == (kept, 1)
    rng = np.random.default_rng(stride)
    idx = rng.integers(0, len(xyz), 777).astype(np.int32)                          # repeats, any order
    out, kept = dc.extract_indices(idx)
    assert kept == 777 and _download_words(out, stride, ctx).tobytes() == src[idx].tobytes() and out.info()[2:4] == (777, 1)
    keep = np.ones(len(xyz), bool)
    keep[idx] = False
    out, kept = dc.extract_indices(idx, negative=True)
    assert kept == keep.sum() and _download_words(out, stride, ctx).tobytes() == src[keep].tobytes()


def test_plane_filter_keep_organized_and_in_place(api, ctx):
    xyz = LC.non_finite_xyz()
    cloud = CK.cloud(xyz)
    cloud = type(cloud)(cloud.points, 60, 50, False)
    model, thr = np.array([0.6, 0.0, 0.8, -0.1], np.float32), 0.2
    inl = R.within(model, xyz, thr)[0]
    src = cloud.points.view(np.uint32).reshape(len(xyz), 8)
    for negative in (False, True):
        keep = inl != negative
        out, kept = api.DeviceCloud(cloud, ctx=ctx).plane_filter(model, thr, negative=negative, keep_organized=True)
        got = out.download()
        assert kept == keep.sum() and (len(got), got.width, got.height, bool(got.is_dense)) == (len(xyz), 60, 50, False)
        raw = got.points.view(np.uint32).reshape(len(xyz), 8)
        assert (raw[~keep, :3] == QNAN).all() and (raw[~keep, 3:] == src[~keep, 3:]).all() and raw[keep].tobytes() == src[keep].tobytes()
    dc = api.DeviceCloud(cloud, ctx=ctx)
    stamp = dc.stamp
    same, kept = dc.plane_filter(model, thr, out=dc)                               # in == out
    assert same is dc and kept == inl.sum() == len(dc) and dc.stamp[1] != stamp[1] and dc.download().points.tobytes() == _rec(cloud.points, inl)
    empty, kept = api.DeviceCloud(_cloud(np.zeros((0, 3), np.float32)), ctx=ctx).plane_filter(model, thr)
    assert kept == 0 and len(empty) == 0
    everything, kept = api.DeviceCloud(cloud, ctx=ctx).plane_filter([0, 0, 0, 0], 1.0)      # a zero normal: every finite record
    assert kept == np.isfinite(xyz).all(axis=1).sum()


def test_extract_indices_lists_and_refusals(api, ctx):
    from rsreg_amd import lib
    L = lib.lib()
    xyz = K.count_cloud(500)
    cloud = _cloud(xyz)
    dc = api.DeviceCloud(cloud, ctx=ctx)
    out, kept = dc.extract_indices([])                                             # an empty list: nothing, or everything
    assert kept == 0 and len(out) == 0
    out, kept = dc.extract_indices([], negative=True)
    assert kept == 500 and out.download().points.tobytes() == cloud.points.tobytes()
    full = np.arange(500, dtype=np.int32)
    out, kept = dc.extract_indices(full[::-1])                                     # the full list, reversed
    assert kept == 500 and out.download().points.tobytes() == _rec(cloud.points, slice(None, None, -1))
    out, kept = dc.extract_indices(full, negative=True)
    assert kept == 0 and len(out) == 0
    rep = np.array([7, 7, 7, 499, 0, 7], np.int32)                                 # repeats
    out, kept = dc.extract_indices(rep)
    assert kept == 6 and out.download().points.tobytes() == _rec(cloud.points, rep)
    out, kept = dc.extract_indices(rep, negative=True)
    assert kept == 497
    grown = np.tile(full, 3)                                                       # more records than the input holds, in place
    twin = api.DeviceCloud(cloud, ctx=ctx)
    same, kept = twin.extract_indices(grown, out=twin)
    assert same is twin and kept == 1500 == len(twin) and twin.download().points.tobytes() == _rec(cloud.points, grown)
    target = api.DeviceCloud(_cloud(K.count_cloud(9)), ctx=ctx)
    before, stamp = target.download().points.tobytes(), target.stamp
    n_kept = C.c_uint64(99)
    for bad in ([500], [-1], [3, 4, 2 ** 31 - 1], [0, 1, -2 ** 31]):                   # an index outside the cloud, checked on the host
        idx = np.array(bad, np.int32)
        for negative in (0, 1):
            assert L.rsreg_cloud_extract_indices(ctx.h, dc.h, idx.ctypes.data, len(idx), negative, target.h, C.byref(n_kept)) == lib.RSREG_ERR_INVALID_ARG
    assert L.rsreg_cloud_extract_indices(ctx.h, dc.h, None, 3, 0, target.h, C.byref(n_kept)) == lib.RSREG_ERR_INVALID_ARG
    assert L.rsreg_cloud_extract_indices(ctx.h, dc.h, full.ctypes.data, 3, 0, None, C.byref(n_kept)) == lib.RSREG_ERR_INVALID_ARG
    other = api.Context(0)
    foreign = api.DeviceCloud(ctx=other)
    assert L.rsreg_cloud_extract_indices(ctx.h, dc.h, full.ctypes.data, 3, 0, foreign.h, C.byref(n_kept)) == lib.RSREG_ERR_INVALID_ARG
    assert L.rsreg_cloud_plane_filter(ctx.h, dc.h, np.zeros(4, np.float32).ctypes.data, 0.1, 0, 0, foreign.h, C.byref(n_kept)) == lib.RSREG_ERR_INVALID_ARG
    assert n_kept.value == 99 and target.download().points.tobytes() == before and target.stamp == stamp and len(foreign) == 0
    lib.check(L.rsreg_cloud_extract_indices(ctx.h, dc.h, full.ctypes.data, 3, 0, target.h, None), ctx.h)      # n_kept may be NULL
    assert target.download().points.tobytes() == _rec(cloud.points, slice(0, 3))


# ------------------------------------------------------------------------------------------------ adaptors
def test_adaptors(api, ctx, tmp_path):
    """tests/cpp/plane_seg_runner.cpp (rsreg::SACSegmentation, rsreg::ExtractIndices) gives the Python classes' results byte for
    byte, from a host cloud and from a device cloud; the Python classes give the device path's."""
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "plane_seg_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "plane_seg_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    for name, perpendicular in (("a60_s1", 0), ("b_axis_z", 1), ("collinear", 0)):
        xyz, prm = _case(name)
        ref = _ref(api, name)
        cloud = _cloud(xyz)
        seg = api.SACSegmentation(ctx=ctx)
        seg.setModelType(api.SACMODEL_PERPENDICULAR_PLANE if perpendicular else api.SACMODEL_PLANE)
        seg.setMethodType(api.SAC_RANSAC)
        seg.setDistanceThreshold(prm["distance_threshold"])
        seg.setMaxIterations(prm.get("max_iterations", 50))
        seg.setSeed(prm["seed"])
        seg.setAxis((0, 0, 1))                                                     # (the plain model ignores it)
        seg.setEpsAngle(prm.get("eps_angle", K.EPS_10_DEG))
        results = []
        for c in (cloud, api.DeviceCloud(cloud, ctx=ctx)):
            seg.setInputCloud(c)
            inliers, coeff = seg.segment()
            _check_segment((coeff, inliers, seg.result), ref, name)
            results.append((inliers, coeff))
        ex = api.ExtractIndices(ctx=ctx)
        ex.setInputCloud(cloud)
        ex.setIndices(results[0][0])
        plane = ex.filter()
        ex.setNegative(True)
        rest = ex.filter()
        keep = np.ones(len(xyz), bool)
        keep[ref.inliers] = False
        assert plane.points.tobytes() == _rec(cloud.points, ref.inliers) and rest.points.tobytes() == _rec(cloud.points, keep)
        assert ex.n_kept == keep.sum()

        cloud.points.tofile(str(tmp_path / "in.bin"))
        prefix = str(tmp_path / (name + "_"))
        r = subprocess.run([exe, str(tmp_path / "in.bin"), str(len(xyz)), repr(prm["distance_threshold"]), str(prm.get("max_iterations", 50)), str(prm["seed"]),
                            "1", str(perpendicular), repr(prm.get("eps_angle", K.EPS_10_DEG)), prefix], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout
        vals = dict(l.split() for l in r.stdout.strip().splitlines())
        assert int(vals["inliers"]) == int(vals["inliers_device"]) == ref.n_inliers and int(vals["rest"]) == keep.sum()
        assert (int(vals["iterations"]), int(vals["skipped"])) == (ref.iterations, ref.skipped)
        for where in ("host_", "dev_"):
            assert np.fromfile(prefix + where + "inliers.bin", np.int32).tobytes() == ref.inliers.tobytes()
            coeff = np.fromfile(prefix + where + "coeff.bin", np.float32)
            assert coeff.tobytes() == (np.asarray(ref.coeff, np.float32).tobytes() if ref.found else b"")
            assert open(prefix + where + "plane.bin", "rb").read() == plane.points.tobytes()
            assert open(prefix + where + "rest.bin", "rb").read() == rest.points.tobytes()
