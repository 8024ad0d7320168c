"""rsreg_cloud_euclidean_clusters and rsreg_cloud_cluster_filter (pcl::EuclideanClusterExtraction) on the GPU, the Python and C++
adaptors, against tests/cluster_ref.py.

The result is a set partition with a total order on its parts, so every check is an EQUALITY: labels, indices, offsets and the number
of clusters are the reference's, whatever order the device linked the edges in.  The inputs (tests/cluster_cases.py): the lattice puts
records AT the tolerance (1 728 singletons: rank = record index) and just inside it, the pile puts a cell's run beyond a wave, r = 10
holds the whole cloud in one ball, the snakes are one component whose diameter is about its size (the deep-tree case of a union-find;
the large one has more records than a walk launch has workgroups), the blobs tie three clusters of 400 and 60 singletons.  The
expected partition of the large snakes and of r = 10 comes from the construction (tests/test_clusters_cpu.py holds the reference
against it); every other one from PCL's seed loop over radius_ref's adjacency.

Not run here: the refusal of a cloud of 2^30 records or more (13 GB of records to get to a check in front of every launch).
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import cluster_cases as K
import cluster_ref as CR
import layout_cases as LC
import radius_cases as RC
import radius_ref as R
import sor_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QNAN = 0x7fc00000
CANARY = 0xA5A5A5A5
U32_MAX = 2 ** 32 - 1
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


@functools.lru_cache(maxsize=None)
def _search(name, tol):
    return R.search(K.input_cloud(name).xyz, tol)


@functools.lru_cache(maxsize=None)
def _ref(name, tol, min_size=1, max_size=CR.INT_MAX):
    n = len(K.input_cloud(name))
    if name == "uniform5000" and tol == 10.0:            # the box's diagonal is 2.6: one ball holds the cloud (25 M candidates for the tree)
        return CR.from_groups(np.zeros(n, np.int64), min_size, max_size)
    if name.startswith("snake_large"):                   # from the construction (tests/test_clusters_cpu.py: it is the reference's)
        group = K.snake_groups(*K.SNAKE_LARGE, cut=K.SNAKE_CUT if name.endswith("cut") else None)[1]
        return CR.from_groups(group if tol == K.R_FACE else np.arange(n), min_size, max_size)
    return CR.extract(K.input_cloud(name).xyz, tol, min_size, max_size, nb=_search(name, tol))


class _Got:
    pass


def _call(dc, tol, min_size=1, max_size=CR.INT_MAX, capacity=None, want=("labels", "indices", "offsets", "count"), expect=0):
    """rsreg_cloud_euclidean_clusters into buffers filled with a canary, eight words longer than the contract asks for."""
    from rsreg_amd import lib
    n = dc.info()[0]
    capacity = n if capacity is None else capacity
    g = _Got()
    g.labels, g.indices, g.offsets = (np.full(m + 8, CANARY, np.uint32) for m in (n, n, min(n, capacity) + 1))
    count = C.c_uint32(CANARY)
    p = lib.ClusterParams(float(tol), int(min_size), int(max_size))
    rc = lib.lib().rsreg_cloud_euclidean_clusters(dc.ctx.h, dc.h, C.byref(p), *(getattr(g, k).ctypes.data if k in want else None
                                                                               for k in ("labels", "indices", "offsets")),
                                                  capacity, C.byref(count) if "count" in want else None)
    assert rc == expect, (rc, lib.lib().rsreg_last_error(dc.ctx.h))
    g.count = count.value
    return g


def _check(g, ref, n, capacity=None, want=("labels", "indices", "offsets", "count")):
    """Every array the call was given equals the reference's, and nothing behind what the contract writes was touched."""
    reported = ref.n_clusters if capacity is None else min(ref.n_clusters, capacity)
    listed = int(ref.offsets[reported])
    if "count" in want:
        assert g.count == ref.n_clusters
    if "labels" in want:
        np.testing.assert_array_equal(g.labels[:n].view(np.int32), ref.labels)
    if "offsets" in want:
        np.testing.assert_array_equal(g.offsets[:reported + 1], ref.offsets[:reported + 1])
    if "indices" in want:
        np.testing.assert_array_equal(g.indices[:listed], ref.indices[:listed])
    for k, written in (("labels", n), ("offsets", reported + 1), ("indices", listed)):
        assert (getattr(g, k)[written if k in want else 0:] == CANARY).all(), k


def _records(points, mask):
    return np.ascontiguousarray(points).view(np.uint8).reshape(len(points), -1)[mask].tobytes()


# ------------------------------------------------------------------------------------------------ equality with the reference
EQUAL = ([("lattice", K.R_AT), ("lattice", K.R_FACE), ("lattice_pile", K.R_FACE), ("uniform5000", 0.05), ("uniform5000", 0.1), ("uniform5000", 10.0),
          ("sphere5000", 0.03), ("non_finite", 0.1), ("frame_raw", 0.03), ("frame_pass", 0.02), ("frame_pass", 0.01), ("blobs", K.BLOB_TOL)] +
         [(name, tol) for name in ("snake_small", "snake_large") for tol in (K.R_AT, K.R_FACE)] + [("snake_large_cut", K.R_FACE)])


@pytest.mark.parametrize("name,tol", EQUAL)
def test_clusters_equal_the_reference(api, ctx, name, tol):
    cloud = K.input_cloud(name)
    ref = _ref(name, tol)
    g = _call(api.DeviceCloud(cloud, ctx=ctx), tol)
    sizes = np.diff(ref.offsets.astype(np.int64))
    print("clusters: %s, n = %d, tolerance %g: %d clusters (device %d), the largest %d, %d singletons, labels that differ: %d" %
          (name, len(cloud), tol, ref.n_clusters, g.count, sizes.max(), int((sizes == 1).sum()),
           int((g.labels[:len(cloud)].view(np.int32) != ref.labels).sum())))
    _check(g, ref, len(cloud))
    fin = S.finite_rows(cloud.xyz)
    assert (ref.labels[~fin] == -1).all() and (ref.labels[fin] >= 0).all()        # -1 on exactly the non-finite rows


def test_shapes_by_hand(api, ctx):
    n = 1728
    at = _call(api.DeviceCloud(K.input_cloud("lattice"), ctx=ctx), K.R_AT)        # AT the tolerance: not joined
    assert at.count == n and (at.labels[:n] == np.arange(n)).all() and (at.indices[:n] == np.arange(n)).all() and (at.offsets[:n + 1] == np.arange(n + 1)).all()
    pile = _call(api.DeviceCloud(K.input_cloud("lattice_pile"), ctx=ctx), 0.5 * K.H)   # exact copies are joined like any other pair
    assert pile.count == n and pile.offsets[1] == 301 and pile.indices[:301].tolist() == [777] + list(range(n, n + 300))
    sizes = K.snake_sizes(*K.SNAKE_LARGE, K.SNAKE_CUT)
    cut = _call(api.DeviceCloud(K.input_cloud("snake_large_cut"), ctx=ctx), K.R_FACE)
    assert cut.count == 2 and cut.offsets[:3].tolist() == [0, max(sizes), sum(sizes)]
    ref = _ref("blobs", K.BLOB_TOL)                                                  # (each blob one component: on the reference alone)
    assert np.diff(ref.offsets).tolist() == list(K.BLOB_SIZES) + [1] * K.BLOB_ISOLATED
    blobs = _call(api.DeviceCloud(K.input_cloud("blobs"), ctx=ctx), K.BLOB_TOL)
    first = blobs.indices[blobs.offsets[:blobs.count]].astype(np.int64)
    assert (np.diff(first[:3]) > 0).all() and (np.diff(first[6:]) > 0).all()         # ties: the lower smallest record first


# ------------------------------------------------------------------------------------------------ bounds, capacity, small clouds
@pytest.mark.parametrize("min_size,max_size", [(2, CR.INT_MAX), (8, CR.INT_MAX), (41, CR.INT_MAX), (1, 399), (1, 400), (8, 399)])
def test_bounds_drop_whole_components(api, ctx, min_size, max_size):
    cloud = K.input_cloud("blobs")
    every, ref = _ref("blobs", K.BLOB_TOL), _ref("blobs", K.BLOB_TOL, min_size, max_size)
    g = _call(api.DeviceCloud(cloud, ctx=ctx), K.BLOB_TOL, min_size, max_size)
    _check(g, ref, len(cloud))
    sizes = np.diff(every.offsets.astype(np.int64))
    inside = (sizes >= min_size) & (sizes <= max_size)
    assert g.count == int(inside.sum()) and (g.count < every.n_clusters) == (max_size < 400 or min_size > 1)   # the ranks close up
    dropped = np.isin(every.labels, np.flatnonzero(~inside))
    labels = g.labels[:len(cloud)].view(np.int32)
    assert (labels[dropped] == -1).all() and (labels[~dropped] >= 0).all()           # a component is dropped whole, never split
    assert sorted(np.unique(labels[~dropped]).tolist()) == list(range(g.count))


def test_capacity_and_nullable_outputs(api, ctx):
    cloud, tol = K.input_cloud("uniform5000"), 0.05
    ref, dc, n = _ref("uniform5000", tol), api.DeviceCloud(cloud, ctx=ctx), len(cloud)
    for capacity in (0, 1, 7, ref.n_clusters - 1, ref.n_clusters, ref.n_clusters + 1):
        _check(_call(dc, tol, capacity=capacity), ref, n, capacity)                  # the count is the full one
    every = ("labels", "indices", "offsets", "count")
    for missing in every:
        want = tuple(k for k in every if k != missing)
        _check(_call(dc, tol, capacity=7, want=want), ref, n, 7, want)
    _check(_call(dc, tol, want=("count",)), ref, n, want=("count",))
    _check(_call(dc, tol, want=()), ref, n, want=())


def test_small_clouds(api, ctx):
    one = _call(api.DeviceCloud(K.input_cloud("one"), ctx=ctx), 0.5)                 # one finite record among NaNs
    assert one.count == 1 and one.labels[:9].view(np.int32).tolist() == [-1] * 4 + [0] + [-1] * 4
    assert one.indices[:1].tolist() == [4] and one.offsets[:2].tolist() == [0, 1] and (one.indices[1:] == CANARY).all()
    assert _call(api.DeviceCloud(K.input_cloud("one"), ctx=ctx), 0.5, min_size=2).count == 0
    none = _call(api.DeviceCloud(K.input_cloud("none_finite"), ctx=ctx), 0.5)        # no finite record: nothing is launched
    assert none.count == 0 and (none.labels[:70].view(np.int32) == -1).all() and (none.labels[70:] == CANARY).all()
    assert none.offsets[0] == 0 and (none.offsets[1:] == CANARY).all() and (none.indices == CANARY).all()
    empty = _call(api.DeviceCloud(K.input_cloud("empty"), ctx=ctx), 0.5)
    assert empty.count == 0 and empty.offsets[0] == 0 and (empty.offsets[1:] == CANARY).all() and (empty.labels == CANARY).all()
    labels, indices, offsets = api.DeviceCloud(K.input_cloud("none_finite"), ctx=ctx).euclidean_clusters(0.5)
    assert (labels == -1).all() and len(indices) == 0 and offsets.tolist() == [0]
    _check(_call(api.DeviceCloud(K.input_cloud("lattice"), ctx=ctx), K.R_FACE), _ref("lattice", K.R_FACE), 1728)   # ... and the context goes on


@pytest.mark.parametrize("name,tol", [("uniform5000", 0.05), ("snake_large", K.R_FACE), ("frame_raw", 0.03)])
def test_same_bytes_from_any_context(api, ctx, name, tol):
    cloud = K.input_cloud(name)
    dc = api.DeviceCloud(cloud, ctx=ctx)
    a, b = _call(dc, tol), _call(dc, tol)
    other = api.Context(0)
    api.DeviceCloud(K.input_cloud("sphere5000"), ctx=other).radius_count(0.2)        # the fresh context has indexed another cloud first
    c = _call(api.DeviceCloud(cloud, ctx=other), tol)
    for g in (b, c):
        assert g.count == a.count
        for k in ("labels", "indices", "offsets"):
            assert getattr(g, k).tobytes() == getattr(a, k).tobytes(), k
    _check(a, _ref(name, tol), len(cloud))


# ------------------------------------------------------------------------------------------------ cluster_filter
FILTER = [("blobs", K.BLOB_TOL), ("frame_pass", 0.02), ("non_finite", 0.1)]
RANGES = [(0, 1, 1), (1, 3, 1), (0, U32_MAX, 8)]


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("rank_lo,rank_hi,min_size", RANGES)
@pytest.mark.parametrize("name,tol", FILTER)
def test_filter_keeps_the_reference_records(api, ctx, name, tol, rank_lo, rank_hi, min_size, negative):
    cloud = K.input_cloud(name)
    keep = CR.filter_keep(_ref(name, tol, min_size).labels, rank_lo, rank_hi, negative)
    out, kept = api.DeviceCloud(cloud, ctx=ctx).cluster_filter(tol, rank_lo, rank_hi, min_size=min_size, negative=negative)
    got = out.download()
    print("cluster filter: %s at %g, ranks [%d, %d), min %d, negative %d: kept %d of %d" % (name, tol, rank_lo, rank_hi, min_size, negative, kept, len(cloud)))
    assert kept == int(keep.sum()) == len(got) and 0 < kept < len(cloud)
    assert got.points.tobytes() == _records(cloud.points, keep)
    assert (got.width, got.height, bool(got.is_dense)) == (kept, 1, bool(cloud.is_dense))


def test_filter_keep_organized(api, ctx):
    cloud = K.input_cloud("non_finite")
    for dense_in in (True, False):
        cloud = type(cloud)(cloud.points, cloud.width, cloud.height, dense_in)
        for (rank_lo, rank_hi, min_size), negative in ((RANGES[0], False), (RANGES[1], True), (RANGES[2], False)):
            keep = CR.filter_keep(_ref("non_finite", 0.1, min_size).labels, rank_lo, rank_hi, negative)
            out, kept = api.DeviceCloud(cloud, ctx=ctx).cluster_filter(0.1, rank_lo, rank_hi, min_size=min_size, negative=negative, keep_organized=True)
            got = out.download()
            assert kept == int(keep.sum()) and 0 < kept < len(cloud)
            assert (len(got), got.width, got.height, bool(got.is_dense)) == (len(cloud), 60, 50, False)    # something was removed
            raw, src = got.points.view(np.uint32).reshape(len(cloud), 8), cloud.points.view(np.uint32).reshape(len(cloud), 8)
            assert (raw[~keep, :3] == QNAN).all() and (raw[~keep, 3:] == src[~keep, 3:]).all()
            assert raw[keep].tobytes() == src[keep].tobytes()
    full = type(cloud)(K.input_cloud("uniform1000").points, 40, 25, True)                                  # nothing is removed
    out, kept = api.DeviceCloud(full, ctx=ctx).cluster_filter(10.0, keep_organized=True)
    got = out.download()
    assert kept == 1000 and (got.width, got.height, bool(got.is_dense)) == (40, 25, True) and got.points.tobytes() == full.points.tobytes()


def test_filter_in_place_and_nullable_count(api, ctx):
    from rsreg_amd import lib
    L = lib.lib()
    cloud = K.input_cloud("blobs")
    want = _records(cloud.points, CR.filter_keep(_ref("blobs", K.BLOB_TOL).labels, 1, 3))
    dc = api.DeviceCloud(cloud, ctx=ctx)
    stamp = dc.stamp
    same, kept = dc.cluster_filter(K.BLOB_TOL, 1, 3, out=dc)                                               # in == out
    assert same is dc and kept == len(want) // 32 == len(dc) == 800 and dc.stamp[1] != stamp[1]
    assert dc.download().points.tobytes() == want
    src, out = api.DeviceCloud(cloud, ctx=ctx), api.DeviceCloud(ctx=ctx)
    p = api.cluster_params(K.BLOB_TOL)
    lib.check(L.rsreg_cloud_cluster_filter(ctx.h, src.h, C.byref(p), 1, 3, 0, 0, out.h, None), ctx.h)      # n_kept may be NULL
    assert out.download().points.tobytes() == want
    lib.check(L.rsreg_cloud_cluster_filter(ctx.h, src.h, C.byref(p), 2, 2, 0, 0, out.h, None), ctx.h)      # an empty range keeps nothing
    assert len(out) == 0
    empty, kept = api.DeviceCloud(K.input_cloud("empty"), ctx=ctx).cluster_filter(0.05)
    assert kept == 0 and len(empty) == 0
    none, kept = api.DeviceCloud(K.input_cloud("none_finite"), ctx=ctx).cluster_filter(0.05, negative=True)   # label -1: outside every range
    assert kept == 70 and none.download().points.tobytes() == K.input_cloud("none_finite").points.tobytes()
    none, kept = api.DeviceCloud(K.input_cloud("none_finite"), ctx=ctx).cluster_filter(0.05, 0, U32_MAX)
    assert kept == 0 and len(none) == 0


# ------------------------------------------------------------------------------------------------ record layouts
@pytest.mark.parametrize("stride", [12, 48])
def test_record_layouts(api, ctx, stride):
    xyz = LC.non_finite_xyz()
    ref = _ref("non_finite", 0.1)
    src = LC.words(xyz, stride)
    dc = api.DeviceCloud(LC.raw_cloud(xyz, stride, 60, 50), ctx=ctx)
    _check(_call(dc, 0.1), ref, len(xyz))
    keep = CR.filter_keep(ref.labels, 0, 1)
    out, kept = dc.cluster_filter(0.1)
    n, got_stride = out.info()[:2]
    buf = np.zeros((n, stride // 4), np.uint32)
    from rsreg_amd import lib
    lib.check(lib.lib().rsreg_cloud_download(out.h, buf.ctypes.data, n), ctx.h)
    assert (n, got_stride, kept) == (int(keep.sum()), stride, int(keep.sum())) and buf.tobytes() == src[keep].tobytes()


# ------------------------------------------------------------------------------------------------ errors
def test_errors_leave_everything_unchanged(api, ctx):
    from rsreg_amd import lib
    L = lib.lib()
    xyz = RC.uniform(40, 8)
    dc = api.DeviceCloud(K.cloud(xyz), ctx=ctx)
    out = api.DeviceCloud(K.cloud(RC.uniform(7, 9)), ctx=ctx)
    before, stamp = out.download().points.tobytes(), out.stamp
    inv = lib.RSREG_ERR_INVALID_ARG
    kept = C.c_uint64(99)
    other = api.Context(0)
    foreign_in, foreign_out = api.DeviceCloud(K.cloud(xyz), ctx=other), api.DeviceCloud(ctx=other)

    def clusters(cloud_h, p):
        g = _Got()
        g.labels, g.indices, g.offsets = (np.full(48, CANARY, np.uint32) for _ in range(3))
        count = C.c_uint32(CANARY)
        rc = L.rsreg_cloud_euclidean_clusters(ctx.h, cloud_h, None if p is None else C.byref(p), g.labels.ctypes.data, g.indices.ctypes.data,
                                              g.offsets.ctypes.data, 40, C.byref(count))
        assert rc == inv
        assert count.value == CANARY and all((a == CANARY).all() for a in (g.labels, g.indices, g.offsets))

    def filt(in_h, p, lo, hi, out_h, organized=0):
        assert L.rsreg_cloud_cluster_filter(ctx.h, in_h, None if p is None else C.byref(p), lo, hi, 0, organized, out_h, C.byref(kept)) == inv

    good = lib.ClusterParams(0.1, 1, CR.INT_MAX)
    for bad in (0.0, -0.03, float("nan"), float("inf"), float("-inf")):
        p = lib.ClusterParams(bad, 1, CR.INT_MAX)
        clusters(dc.h, p)
        filt(dc.h, p, 0, 1, out.h)
        filt(dc.h, p, 0, 1, out.h, 1)
    p = lib.ClusterParams(0.1, 5, 4)                          # min_cluster_size > max_cluster_size
    clusters(dc.h, p)
    filt(dc.h, p, 0, 1, out.h)
    filt(dc.h, good, 2, 1, out.h)                             # rank_lo > rank_hi
    clusters(dc.h, None)                                      # NULL p, in, out
    filt(dc.h, None, 0, 1, out.h)
    clusters(None, good)
    filt(None, good, 0, 1, out.h)
    filt(dc.h, good, 0, 1, None)
    clusters(foreign_in.h, good)                              # a cloud of another context
    filt(foreign_in.h, good, 0, 1, out.h)
    filt(dc.h, good, 0, 1, foreign_out.h)
    assert out.download().points.tobytes() == before and out.stamp == stamp and len(dc) == 40
    assert kept.value == 99 and len(foreign_out) == 0
    with pytest.raises(lib.RsregError) as e:
        dc.euclidean_clusters(0.0)
    assert e.value.status == inv
    with pytest.raises(lib.RsregError) as e:
        dc.cluster_filter(0.1, 3, 2)
    assert e.value.status == inv
    ref = CR.extract(xyz, 0.3)                                # ... and the calls that are right
    _check(_call(dc, 0.3), ref, 40)
    _, n_kept = dc.cluster_filter(0.3, out=out)
    assert out.stamp[1] != stamp[1] and n_kept == int(np.diff(ref.offsets)[0]) == len(out)
    assert L.rsreg_version() == 4


# ------------------------------------------------------------------------------------------------ adaptors
def _runner_clusters(path):
    words = np.fromfile(path, np.int32)
    out, at = [], 1
    for _ in range(int(words[0])):
        m = int(words[at])
        out.append(words[at + 1:at + 1 + m])
        at += 1 + m
    assert at == len(words)
    return out


def test_adaptors(api, ctx, tmp_path):
    """tests/cpp/cluster_runner.cpp gives the clusters of the Python device path, list for list, from a host cloud and from a device
    cloud; so does api.EuclideanClusterExtraction on a host cloud."""
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "cluster_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cluster_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    fr, tol, min_size, max_size = K.input_cloud("frame_raw"), 0.03, 2, 30000
    ref = _ref("frame_raw", tol, min_size, max_size)
    labels, indices, offsets = api.DeviceCloud(fr, ctx=ctx).euclidean_clusters(tol, min_size, max_size)
    assert labels.dtype == np.int32 and indices.dtype == np.uint32 and offsets.dtype == np.uint32
    assert labels.tobytes() == ref.labels.tobytes() and indices.tobytes() == ref.indices.tobytes() and offsets.tobytes() == ref.offsets.tobytes()
    assert 0 < ref.n_clusters < _ref("frame_raw", tol).n_clusters                    # both bounds drop something
    want = [indices[offsets[c]:offsets[c + 1]].astype(np.int32) for c in range(len(offsets) - 1)]

    ec = api.EuclideanClusterExtraction()
    ec.setInputCloud(fr)                                      # a host cloud: through a temporary DeviceCloud
    ec.setClusterTolerance(tol)
    ec.setMinClusterSize(min_size)
    ec.setMaxClusterSize(max_size)
    for cloud in (fr, api.DeviceCloud(fr, ctx=ctx)):
        ec.setInputCloud(cloud)
        got = ec.extract()
        assert len(got) == len(want) and all(a.dtype == np.int32 and a.tobytes() == b.tobytes() for a, b in zip(got, want))

    fr.points.tofile(str(tmp_path / "in.bin"))
    names = ["clusters_host.bin", "clusters_dev.bin"]
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(fr.width), str(fr.height), repr(tol), str(min_size), str(max_size)] +
                       [str(tmp_path / f) for f in names], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    vals = dict(l.split() for l in r.stdout.strip().splitlines())
    assert int(vals["clusters"]) == int(vals["clusters_device"]) == len(want)
    for f in names:
        got = _runner_clusters(str(tmp_path / f))
        assert len(got) == len(want) and all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), f
