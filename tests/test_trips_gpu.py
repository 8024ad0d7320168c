"""The one-wave-per-query kernels of csrc/filters.hip past one launch's workgroups: k_knn_indices (rsreg_cloud_knn), k_normals
(rsreg_cloud_normals), k_radius_count (rsreg_cloud_radius_count, rsreg_cloud_radius_outlier_removal) and k_normals_radius
(rsreg_cloud_normals_radius) run min(nfin, 65 536) workgroups with a grid-stride loop over the queries in cell order.  On the clouds
of tests/trips_cases.py a workgroup answers two, three and four queries (the largest trip count reached: 4): the LDS selection
buffer is appended to again behind the barrier, k_normals_radius takes its `continue` on fewer than three neighbours and goes on,
and record ids pass 65 535.  tests/test_trips_cpu.py holds what the clouds claim.

Every expected value comes from tests/normals_ref.py and tests/radius_ref.py, computed once per case:
  * knn(k): indices and d2 BIT-EQUAL to normals_ref.knn on every row, -1 / 0 in the rows of non-finite records; by hand, the
    k = 64 neighbours of every record of a pile are the 64 lowest record indices in that place;
  * normals(k): every rule of tests/test_normals_gpu.py::_check_normals, imported unchanged; the 5 % cap on the share left out is
    asserted on every case (two_trips_piles: 0.91 %, the piles, whose neighbours all lie in one place; the others 0.00 %);
  * radius_count(r): EQUAL to radius_ref.counts on every record; normals_radius(r): NaN rows exactly where the count is below 3,
    the normals under the rules of tests/test_radius_gpu.py::_check_normals, imported unchanged; RadiusOutlierRemoval with
    min_neighbors = 2, negative both ways: the records of radius_ref.ror_keep, byte for byte and in order;
  * knn and normals of two_trips_piles from a second, fresh context: the same bytes.
"""
import functools
import time

import numpy as np
import pytest

import normals_ref as N
import radius_ref as R
import sor_ref as S
import trips_cases as T
from test_normals_gpu import _check_normals
from test_radius_gpu import _check_normals as _check_normals_radius

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
    print("\ntrips: %.1f s from the first context to the last test" % (time.perf_counter() - t0))


_DEV = {}


def _dc(api, ctx, name):
    """The case's DeviceCloud on the module's context, uploaded once."""
    if name not in _DEV:
        _DEV[name] = api.DeviceCloud(T.cloud(name), ctx=ctx)
    return _DEV[name]


@functools.lru_cache(maxsize=None)
def _ref_knn(name, k):
    return N.knn(T.xyz(name), k)


@functools.lru_cache(maxsize=None)
def _ref_normals(name, k):
    return N.normals(T.xyz(name), k, (0.0, 0.0, 0.0), knn_result=_ref_knn(name, k))


@functools.lru_cache(maxsize=None)
def _ref_search(name, radius):
    return R.search(T.xyz(name), radius)


@functools.lru_cache(maxsize=None)
def _ref_counts(name, radius):
    return _ref_search(name, radius).counts()


@functools.lru_cache(maxsize=None)
def _ref_normals_radius(name, radius):
    return R.normals(T.xyz(name), radius, (0.0, 0.0, 0.0), nb=_ref_search(name, radius))


def _records(points, mask):
    """All 32 bytes of the records of `points` that `mask` takes, in order."""
    return np.ascontiguousarray(points).view(np.uint8).reshape(len(points), -1)[mask].tobytes()


# ------------------------------------------------------------------------------------------------ the index search
KNN = [("two_trips_piles", 1), ("two_trips_piles", 10), ("two_trips_piles", 64), ("launch_edge_65535", 10), ("launch_edge_65536", 10),
       ("launch_edge_65537", 10), ("four_trips", 10)]


@pytest.mark.parametrize("name,k", KNN)
def test_knn_bit_equal(api, ctx, name, k):
    xyz = T.xyz(name)
    idx, d2 = _dc(api, ctx, name).knn(k)
    want_idx, want_d2 = _ref_knn(name, k)
    assert idx.shape == d2.shape == (len(xyz), k) and idx.dtype == np.int32 and d2.dtype == np.float32
    bad = np.flatnonzero((idx != want_idx).any(axis=1) | (d2.view(np.uint32) != want_d2.view(np.uint32)).any(axis=1))
    first = T.cell_order_positions(xyz)[0]
    print("knn: %s, n = %d, nfin = %d, k = %d, trips %d, rows that differ: %d (of them answered in a later trip: %d)" %
          (name, len(xyz), T.NFIN[name], k, T.trips(T.NFIN[name]), len(bad), int((first[bad] >= T.LAUNCH_CAP).sum())))
    assert len(bad) == 0, (bad[:4], idx[bad[:4]], want_idx[bad[:4]], d2[bad[:4]], want_d2[bad[:4]])
    fin = S.finite_rows(xyz)
    assert int(fin.sum()) == T.NFIN[name]
    assert (idx[~fin] == -1).all() and (d2[~fin] == 0).all()


def test_knn_piles_by_hand(api, ctx):
    """k = 64 of 300 records in one place: the 64 lowest record indices of that place, for every one of them, at distance 0 -- the
    first pile answered in trip 1 (its workgroups go on to trip 2), the second in trip 2."""
    idx, d2 = _dc(api, ctx, "two_trips_piles").knn(64)
    for pile in T.piles():
        assert (idx[pile] == pile[:64].astype(np.int32)).all() and (d2[pile] == 0).all()


# ------------------------------------------------------------------------------------------------ the normals by k
NORMALS = [("two_trips_piles", 10, True), ("two_trips_piles", 64, True), ("launch_edge_65537", 10, True), ("four_trips", 10, True)]


@pytest.mark.parametrize("name,k,share", NORMALS)
def test_normals_against_the_reference(api, ctx, name, k, share):
    cloud = T.cloud(name)
    got = _dc(api, ctx, name).normals(k)
    assert got.shape == (len(cloud), 4) and got.dtype == np.float32
    _check_normals(got, cloud, _ref_normals(name, k), (0.0, 0.0, 0.0), share, "%s k=%d" % (name, k))
    if name == "two_trips_piles":                             # the piles: trace 0, (0, 0, 1) flipped towards the origin, curvature 0
        for pile in T.piles():
            assert (got[pile] == np.float32([0, 0, -1, 0])).all()


# ------------------------------------------------------------------------------------------------ the radius search
RADIUS = [(n, r) for n in ("two_trips_piles", "launch_edge_65537", "four_trips") for r in T.RADII[n]]


@pytest.mark.parametrize("name,radius", RADIUS)
def test_radius_counts_equal_the_reference(api, ctx, name, radius):
    xyz = T.xyz(name)
    got = _dc(api, ctx, name).radius_count(radius)
    want = _ref_counts(name, radius)
    fin = S.finite_rows(xyz)
    print("radius count: %s, n = %d, r = %g, counts %d .. %d, fewer than three: %d, rows that differ: %d" %
          (name, len(xyz), radius, want[fin].min(), want[fin].max(), int((want[fin] < 3).sum()), int((got != want).sum())))
    assert got.dtype == np.uint32 and got.shape == (len(xyz),)
    np.testing.assert_array_equal(got, want)
    assert (got[fin] >= 1).all() and (got[~fin] == 0).all()
    if name == "two_trips_piles":
        for pile in T.piles():
            assert (got[pile] >= T.PILE).all()


@pytest.mark.parametrize("name,radius", RADIUS)
def test_normals_radius_against_the_reference(api, ctx, name, radius):
    cloud = T.cloud(name)
    got = _dc(api, ctx, name).normals_radius(radius)
    assert got.shape == (len(cloud), 4) and got.dtype == np.float32
    ref = _ref_normals_radius(name, radius)
    counts = _ref_counts(name, radius)
    nan = np.isnan(got)
    assert (nan.all(axis=1) == (counts < 3)).all() and (nan.any(axis=1) == nan.all(axis=1)).all()   # NaN rows exactly where m < 3
    assert ((counts < 3) == ~ref.valid).all() and 0 < (counts < 3).sum() < len(cloud)
    _check_normals_radius(got, cloud, ref, (0.0, 0.0, 0.0), True, "%s r=%g" % (name, radius))
    # the `continue`: queries with fewer than three neighbours whose workgroup has another trip to make (all rows are checked above)
    last = T.cell_order_positions(cloud.xyz, "radius", radius)[1]
    go_on = int(((counts < 3) & S.finite_rows(cloud.xyz) & (last < T.NFIN[name] - T.LAUNCH_CAP)).sum())
    print("  queries with fewer than three neighbours whose workgroup goes on to another query: %d" % go_on)
    if name == "four_trips" or radius == 0.02:
        assert go_on > 0


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("name,radius", RADIUS)
def test_ror_keeps_the_reference_records(api, ctx, name, radius, negative):
    cloud = T.cloud(name)
    keep = R.ror_keep(_ref_counts(name, radius), 2, negative)
    out, kept = _dc(api, ctx, name).radius_outlier_removal(radius, 2, negative)
    got = out.download()
    print("ror: %s r = %g min 2 negative %d: kept %d of %d" % (name, radius, negative, kept, len(cloud)))
    assert kept == int(keep.sum()) == len(got) and 0 < kept < len(cloud)
    assert got.points.tobytes() == _records(cloud.points, keep)
    assert (got.width, got.height, bool(got.is_dense)) == (kept, 1, bool(cloud.is_dense))


# ------------------------------------------------------------------------------------------------ bytes, on a second context
def test_bytes_from_a_fresh_context(api, ctx):
    cloud = T.cloud("two_trips_piles")
    dc = _dc(api, ctx, "two_trips_piles")
    fresh = api.Context(0)
    there = api.DeviceCloud(cloud, ctx=fresh)
    for k in (10, 64):
        a_idx, a_d2 = dc.knn(k)
        b_idx, b_d2 = there.knn(k)
        assert a_idx.tobytes() == b_idx.tobytes() and a_d2.tobytes() == b_d2.tobytes()
        np.testing.assert_array_equal(a_idx, _ref_knn("two_trips_piles", k)[0])
        assert dc.normals(k).tobytes() == there.normals(k).tobytes()
