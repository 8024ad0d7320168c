"""rsreg_cloud_radius_count, rsreg_cloud_radius_outlier_removal and rsreg_cloud_normals_radius (pcl::RadiusOutlierRemoval and
pcl::NormalEstimation with setRadiusSearch) on the GPU, the Python and C++ adaptors, against tests/radius_ref.py.

The counts: EQUAL to the reference for every record of every input -- float32 d2 < float32(double r * double r), strictly; the
lattice puts records AT the radius, the piles put a cell's run beyond a wave, r = 10 clamps the box at every face, r = 1e-4 leaves
the cell larger than the radius.  RadiusOutlierRemoval: the kept records byte for byte, in order.

The normals, every record with m >= 3 neighbours of every input (h = 2^-22; C_ref, l0_ref .. l2_ref, n_ref, curv_ref from the
reference alone) -- the bounds of tests/test_normals_gpu.py with m in place of k:
  * | |n| - 1 | <= h: a unit vector in double, each component rounded to float (2^-24 relative each);
  * n^T C_ref n - l0_ref <= h * l0_ref + 1e-12 * trace: the Rayleigh quotient, whatever the eigen-gap.  An angle error e adds
    at most e^2 * l2 (float rounding: 3e-15 * trace), the norm (1 +- 2^-23) scales l0, and the two covariances differ by the
    order of their double sums.  That last term is the only one that grows with the neighbourhood: about m * 2^-53 of the second
    moments, and with m <= 5 000 in these inputs (6 558 on the raw frame's pile, whose moments are all 0) it is below 6e-13 of them:
    it stays under the 1e-12 * trace;
  * |curv - curv_ref| <= 2^-23 * curv_ref + 1e-12: both are floats rounded from doubles that differ by about 1e-13 at most;
  * where gap_ratio = (l1 - l0) / l2 >= 1e-3 (on the reference alone): the angle to +-n_ref is at most 2^-22 rad.  Rounding a
    unit vector to float moves it by at most sqrt(3) * 2^-25 = 5.2e-8; a backward-stable double solve over sums that differ by
    6e-13 relative adds about 6e-13 / 1e-3; the bound is four times the first term -- derived, not measured;
  * the share of records with m >= 3 left out by that condition is at most 5 % per input, asserted on the reference (measured
    with the reference alone: sphere5000 0.21 % at r = 0.03 and 0 % at 0.1, uniform5000 0 % at 0.1, frame_pass 0.01 % at 0.03 and
    0.50 % at 0.02, non_finite 0 % at 0.1).  Exempt from the share, not from the checks: the lattice (1 + 6 neighbours are a cube:
    no direction, 57.9 %) and the raw frame (its 6 558 origin records have every neighbour in one place, 13.1 %);
  * the rows with m < 3 and the non-finite rows are NaN, and no other row is: exactly the reference's rows, no share granted;
  * sign: where the reference has |cos_view| > 1e-6 * |v| (and a gap), n . n_ref > 0; everywhere, n does not point away from
    the viewpoint by more than float rounding; a neighbourhood in one place (trace 0) gives (0, 0, 1) before the flip, curvature 0.
The counts on thin, far, piled-up and cell-aligned clouds (the other rules of the grid's layout): tests/test_pointgrid_searches_gpu.py.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import radius_cases as K
import radius_ref as R
import sor_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -22
QNAN = 0x7fc00000
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
def _ref_search(name, radius):
    return R.search(K.input_cloud(name).xyz, radius)


@functools.lru_cache(maxsize=None)
def _ref_counts(name, radius):
    if name == "uniform5000" and radius == 10.0:
        # the box's diagonal is 2.6: the ball holds the cloud, every count is n (the reference agrees on uniform1000:
        # tests/test_radius_cpu.py::test_tree_candidates_against_brute_force; its 25 M candidates here take seconds)
        return np.full(5000, 5000, np.uint32)
    return _ref_search(name, radius).counts()


@functools.lru_cache(maxsize=None)
def _ref_normals(name, radius, viewpoint=(0.0, 0.0, 0.0)):
    return R.normals(K.input_cloud(name).xyz, radius, viewpoint, nb=_ref_search(name, radius))


def _records(points, mask):
    """All 32 bytes of the records of `points` that `mask` takes, in order (through the byte view: numpy's own indexing of a padded
    structured array copies the fields only)."""
    return np.ascontiguousarray(points).view(np.uint8).reshape(len(points), -1)[mask].tobytes()


# ------------------------------------------------------------------------------------------------ the counts
COUNTS = ([("lattice", r) for r in (K.R_AT, K.R_FACE, K.R_SQRT2, K.R_EDGE)] + [("lattice_pile", K.R_FACE)] +
          [(n, r) for n in ("uniform1000", "uniform5000") for r in (0.05, 0.1)] + [("uniform5000", 10.0), ("uniform5000", 1e-4)] +
          [("sphere5000", 0.03), ("sphere5000", 0.1), ("non_finite", 0.1), ("frame_raw", 0.03), ("frame_pass", 0.02), ("frame_pass", 0.03)])


@pytest.mark.parametrize("name,radius", COUNTS)
def test_counts_equal_the_reference(api, ctx, name, radius):
    cloud = K.input_cloud(name)
    got = api.DeviceCloud(cloud, ctx=ctx).radius_count(radius)
    want = _ref_counts(name, radius)
    fin = S.finite_rows(cloud.xyz)
    print("radius count: %s, n = %d, r = %g, counts %d .. %d, rows that differ: %d" %
          (name, len(cloud), radius, want[fin].min(), want[fin].max(), int((got != want).sum())))
    assert got.dtype == np.uint32 and got.shape == (len(cloud),)
    np.testing.assert_array_equal(got, want)
    assert (got[fin] >= 1).all() and (got[~fin] == 0).all()


def test_counts_by_hand_and_small_clouds(api, ctx):
    inner = (5 * 12 + 5) * 12 + 5
    dc = api.DeviceCloud(K.input_cloud("lattice"), ctx=ctx)
    assert [int(dc.radius_count(r)[inner]) for r in (K.R_AT, K.R_FACE, K.R_SQRT2, K.R_EDGE)] == [1, 7, 7, 19]
    pile = api.DeviceCloud(K.input_cloud("lattice_pile"), ctx=ctx).radius_count(K.R_FACE)
    assert (pile[np.r_[777, 1728:2028]] == 301 + 6).all()
    huge = api.DeviceCloud(K.input_cloud("uniform1000"), ctx=ctx).radius_count(1e30)  # r * r is not a float any more: +inf
    assert (huge == 1000).all()
    one = api.DeviceCloud(K.input_cloud("one"), ctx=ctx).radius_count(0.5)          # one finite record among NaNs
    assert one.tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    none = api.DeviceCloud(K.input_cloud("none_finite"), ctx=ctx)
    assert (none.radius_count(0.5) == 0).all() and len(none.radius_count(0.5)) == 70  # no finite record: nothing is launched
    assert len(api.DeviceCloud(K.input_cloud("empty"), ctx=ctx).radius_count(0.5)) == 0
    assert (dc.radius_count(K.R_FACE) == _ref_counts("lattice", K.R_FACE)).all()      # ... and the context goes on


# ------------------------------------------------------------------------------------------------ RadiusOutlierRemoval
ROR = [("uniform5000", 0.05), ("non_finite", 0.1), ("frame_raw", 0.03)]


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("min_neighbors", [0, 2, 10])
@pytest.mark.parametrize("name,radius", ROR)
def test_ror_keeps_the_reference_records(api, ctx, name, radius, min_neighbors, negative):
    cloud = K.input_cloud(name)
    keep = R.ror_keep(_ref_counts(name, radius), min_neighbors, negative)
    out, kept = api.DeviceCloud(cloud, ctx=ctx).radius_outlier_removal(radius, min_neighbors, negative)
    got = out.download()
    print("ror: %s r = %g min %d negative %d: kept %d of %d" % (name, radius, min_neighbors, negative, kept, len(cloud)))
    assert kept == int(keep.sum()) == len(got)
    assert got.points.tobytes() == _records(cloud.points, keep)
    assert (got.width, got.height, bool(got.is_dense)) == (kept, 1, bool(cloud.is_dense))
    if not negative and min_neighbors == 0:
        assert (keep == S.finite_rows(cloud.xyz)).all()                              # every finite record has itself


def test_ror_keep_organized(api, ctx):
    cloud = K.input_cloud("non_finite")
    for dense_in in (True, False):
        cloud = type(cloud)(cloud.points, cloud.width, cloud.height, dense_in)
        for min_neighbors, negative in ((2, False), (2, True), (10, False)):
            keep = R.ror_keep(_ref_counts("non_finite", 0.1), min_neighbors, negative)
            out, kept = api.DeviceCloud(cloud, ctx=ctx).radius_outlier_removal(0.1, min_neighbors, negative, keep_organized=True)
            got = out.download()
            assert kept == int(keep.sum()) and 0 < kept < len(cloud)
            assert (len(got), got.width, got.height, bool(got.is_dense)) == (len(cloud), 60, 50, False)    # something was removed
            raw, src = got.points.view(np.uint32).reshape(len(cloud), 8), cloud.points.view(np.uint32).reshape(len(cloud), 8)
            assert (raw[~keep, :3] == QNAN).all() and (raw[~keep, 3:] == src[~keep, 3:]).all()
            assert raw[keep].tobytes() == src[keep].tobytes()
    full = type(cloud)(K.input_cloud("uniform1000").points, 40, 25, True)                                  # nothing is removed
    out, kept = api.DeviceCloud(full, ctx=ctx).radius_outlier_removal(10.0, 999, keep_organized=True)
    got = out.download()
    assert kept == 1000 and (got.width, got.height, bool(got.is_dense)) == (40, 25, True) and got.points.tobytes() == full.points.tobytes()


def test_ror_in_place_and_nullable_count(api, ctx):
    from rsreg_amd import lib
    L = lib.lib()
    cloud = K.input_cloud("uniform5000")
    want = _records(cloud.points, R.ror_keep(_ref_counts("uniform5000", 0.05), 2))
    dc = api.DeviceCloud(cloud, ctx=ctx)
    stamp = dc.stamp
    same, kept = dc.radius_outlier_removal(0.05, 2, out=dc)                                                # in == out
    assert same is dc and kept == len(want) // 32 == len(dc) and dc.stamp[1] != stamp[1]
    assert dc.download().points.tobytes() == want
    src, out = api.DeviceCloud(cloud, ctx=ctx), api.DeviceCloud(ctx=ctx)
    lib.check(L.rsreg_cloud_radius_outlier_removal(ctx.h, src.h, 0.05, 2, 0, 0, out.h, None), ctx.h)       # n_kept may be NULL
    assert out.download().points.tobytes() == want
    empty, kept = api.DeviceCloud(K.input_cloud("empty"), ctx=ctx).radius_outlier_removal(0.05, 2)
    assert kept == 0 and len(empty) == 0
    none, kept = api.DeviceCloud(K.input_cloud("none_finite"), ctx=ctx).radius_outlier_removal(0.05, 0, negative=True)
    assert kept == 70 and none.download().points.tobytes() == K.input_cloud("none_finite").points.tobytes()


# ------------------------------------------------------------------------------------------------ the normals
def _check_normals(got, cloud, ref, viewpoint, assert_share, label):
    xyz = cloud.xyz
    fin = ref.valid                                           # finite and m >= 3: the rows that carry a normal
    assert (ref.finite == S.finite_rows(xyz)).all()
    assert np.isnan(got[~fin]).all()                          # NaN in exactly the reference's rows ...
    assert np.isfinite(got[fin]).all()                        # ... and nowhere else
    n = got[fin, :3].astype(np.float64)
    curv = got[fin, 3]
    C, w, tr = ref.C[fin], ref.evals[fin], ref.trace[fin]
    norm_err = np.abs(np.linalg.norm(n, axis=1) - 1).max()
    rq = np.einsum("ni,nij,nj->n", n, C, n) - w[:, 0]
    rq_slack = (rq - (EPS * np.abs(w[:, 0]) + 1e-12 * tr)).max()
    cref = ref.curvature[fin].astype(np.float64)
    curv_slack = (np.abs(curv.astype(np.float64) - cref) - (2.0 ** -23 * cref + 1e-12)).max()
    gap_ok = ref.gap[fin] >= 1e-3
    nref = ref.normal[fin].astype(np.float64)
    nref /= np.linalg.norm(nref, axis=1)[:, None]
    nn = n / np.linalg.norm(n, axis=1)[:, None]
    angle = np.arcsin(np.minimum(np.linalg.norm(np.cross(nn, nref), axis=1), 1.0))
    out_share = 1.0 - gap_ok.mean()
    v = (np.asarray(viewpoint, np.float32)[None, :] - xyz[fin]).astype(np.float64)
    vlen = np.linalg.norm(v, axis=1)
    clear = gap_ok & (np.abs(ref.cos[fin].astype(np.float64)) > 1e-6 * vlen)
    towards = (v * n).sum(axis=1)
    print("%s: m %d .. %d, with a normal %d, NaN rows %d, |n|-1 %.3g, Rayleigh slack %.3g, curvature slack %.3g, max angle %.3g rad over %d, "
          "left out %.2f %%, clear sign %d" %
          (label, ref.m[ref.finite].min(), ref.m[ref.finite].max(), int(fin.sum()), int((~fin).sum()), norm_err, rq_slack, curv_slack,
           angle[gap_ok].max() if gap_ok.any() else 0.0, int(gap_ok.sum()), 100 * out_share, int(clear.sum())))
    assert norm_err <= EPS
    assert rq_slack <= 0
    assert curv_slack <= 0
    assert (angle[gap_ok] <= EPS).all()
    if assert_share:
        assert out_share <= 0.05
    assert ((nn[clear] * nref[clear]).sum(axis=1) > 0).all()
    assert (towards >= -1e-6 * vlen).all()
    flat = tr == 0                                            # all m neighbours in one place: (0, 0, 1) before the flip
    if flat.any():
        want = np.where((ref.cos[fin][flat] < 0)[:, None], np.float32([0, 0, -1]), np.float32([0, 0, 1]))
        assert (got[fin][flat, :3] == want).all() and (curv[flat] == 0).all()


# (input, radius, asserts the share left out by the gap condition)
NORMALS = [("sphere5000", 0.03, True), ("sphere5000", 0.1, True), ("uniform5000", 0.1, True), ("frame_pass", 0.03, True),
           ("frame_pass", 0.02, True), ("non_finite", 0.1, True), ("frame_raw", 0.03, False), ("lattice", K.R_FACE, False)]


@pytest.mark.parametrize("name,radius,share", NORMALS)
def test_normals_against_the_reference(api, ctx, name, radius, share):
    cloud = K.input_cloud(name)
    got = api.DeviceCloud(cloud, ctx=ctx).normals_radius(radius)
    assert got.shape == (len(cloud), 4) and got.dtype == np.float32
    ref = _ref_normals(name, radius)
    _check_normals(got, cloud, ref, (0.0, 0.0, 0.0), share, "%s r=%g" % (name, radius))
    if name == "sphere5000" and radius == 0.1:
        assert ref.m[ref.finite].min() >= 24 and ref.m.max() == 81 > 64              # beyond the k-NN cap
    if name == "frame_raw":                                                          # the missing-depth pile: trace 0, not flipped
        pile = (cloud.xyz == 0).all(axis=1)
        assert pile.sum() == 6558 and (ref.m[pile] == 6558).all()
        assert (got[pile] == np.float32([0, 0, 1, 0])).all()


def test_viewpoint_flips_the_expected_subset(api, ctx):
    vp = (0.3, -0.2, 5.0)
    for name, radius in (("sphere5000", 0.1), ("frame_pass", 0.03)):
        cloud = K.input_cloud(name)
        dc = api.DeviceCloud(cloud, ctx=ctx)
        a, b = dc.normals_radius(radius), dc.normals_radius(radius, viewpoint=vp)
        ref_a, ref_b = _ref_normals(name, radius), _ref_normals(name, radius, vp)
        _check_normals(b, cloud, ref_b, vp, True, "%s r=%g viewpoint" % (name, radius))
        ok = ref_a.valid
        flipped = (a[ok, :3] == -b[ok, :3]).all(axis=1) & (a[ok, :3] != b[ok, :3]).any(axis=1)
        same = (a[ok, :3] == b[ok, :3]).all(axis=1)
        assert (flipped | same).all() and (a[ok, 3] == b[ok, 3]).all()
        want = ((ref_a.cos < 0) != (ref_b.cos < 0))[ok]
        clear = ((ref_a.gap >= 1e-3) & (np.abs(ref_a.cos) > 1e-5) & (np.abs(ref_b.cos) > 1e-5))[ok]
        assert (flipped[clear] == want[clear]).all() and flipped.any() and (name != "sphere5000" or not flipped.all())


def test_output_cloud_and_determinism(api, ctx):
    """32-byte records, pads 0, the quiet NaN, is_dense = 0 as soon as a record got NaNs; the same bytes when called twice and from
    a context that has indexed another cloud first -- the piles (300 copies in one cell, the raw frame's 6 558) are where an order
    left to the atomics of the build would show in the last bits of the sums."""
    from rsreg_amd import lib
    for name, radius, dense_in in (("non_finite", 0.1, True), ("sphere5000", 0.1, True), ("sphere5000", 0.1, False), ("sphere5000", 0.03, True),
                                   ("lattice_pile", K.R_EDGE, True), ("frame_raw", 0.03, False)):
        cloud = K.input_cloud(name)
        cloud = type(cloud)(cloud.points, cloud.width, cloud.height, dense_in)
        dc = api.DeviceCloud(cloud, ctx=ctx)
        ne = api.NormalEstimation()
        ne.setInputCloud(dc)
        ne.setRadiusSearch(radius)
        out = ne.compute()
        n, stride, w, h, dense = out.info()
        assert (n, stride, w, h) == (len(cloud), 32, cloud.width, cloud.height)
        rec = out.download_normals().points
        raw = rec.view(np.uint32).reshape(len(cloud), 8)
        assert (raw[:, 3] == 0).all() and (raw[:, 5:] == 0).all()
        nan_rows = np.isnan(rec["normal_x"])
        assert (nan_rows == ~_ref_normals(name, radius).valid).all()
        assert (raw[nan_rows][:, [0, 1, 2, 4]] == QNAN).all()                        # the quiet NaN, four times
        assert bool(dense) == (False if nan_rows.any() else dense_in)
        again = ne.compute().download_normals().points
        assert rec.tobytes() == again.tobytes()
        other = api.Context(0)                               # a context that has indexed a different cloud first
        api.DeviceCloud(K.input_cloud("sphere5000"), ctx=other).normals_radius(0.05)
        fresh = api.DeviceCloud(cloud, ctx=other).normals_radius_cloud(radius).download_normals().points
        assert rec.tobytes() == fresh.tobytes()
        four = dc.normals_radius(radius)
        assert four.tobytes() == np.stack([rec["normal_x"], rec["normal_y"], rec["normal_z"], rec["curvature"]], 1).tobytes()
    assert lib.lib().rsreg_version() == 4


def test_agrees_with_the_knn_path_on_a_pile(api, ctx):
    """Lattice point 777 and 63 copies of it: for these 64 records the neighbours within 0.5 H and the 64 nearest neighbours are
    the same set, all in one place -- both calls give (0, 0, +-1), curvature 0, and the same bytes."""
    cloud = K.input_cloud("lattice_copies64")
    assert len(cloud) == 1728 + 63
    pile = np.r_[777, 1728:1791]
    dc = api.DeviceCloud(cloud, ctx=ctx)
    assert (dc.radius_count(0.5 * K.H)[pile] == 64).all()
    by_radius, by_k = dc.normals_radius(0.5 * K.H)[pile], dc.normals(64)[pile]
    for got in (by_radius, by_k):
        assert (got[:, :2] == 0).all() and (np.abs(got[:, 2]) == 1).all() and (got[:, 3] == 0).all()
    assert by_radius.tobytes() == by_k.tobytes() and (by_radius[:, 2] == -1).all()   # seen from the origin: flipped


def test_errors_leave_out_unchanged(api, ctx):
    from rsreg_amd import lib
    L = lib.lib()
    xyz = K.uniform(40, 8)
    dc = api.DeviceCloud(K.cloud(xyz), ctx=ctx)
    out = api.DeviceCloud(K.cloud(K.uniform(7, 9)), ctx=ctx)
    before, stamp = out.download().points.tobytes(), out.stamp
    inv = lib.RSREG_ERR_INVALID_ARG
    counts = np.full(40, 77, np.uint32)
    kept = C.c_uint64(99)
    for bad in (0.0, -0.03, float("nan"), float("inf"), float("-inf")):
        assert L.rsreg_cloud_radius_count(ctx.h, dc.h, bad, counts.ctypes.data) == inv
        assert L.rsreg_cloud_radius_outlier_removal(ctx.h, dc.h, bad, 2, 0, 0, out.h, C.byref(kept)) == inv
        assert L.rsreg_cloud_radius_outlier_removal(ctx.h, dc.h, bad, 2, 0, 1, out.h, C.byref(kept)) == inv
        assert L.rsreg_cloud_normals_radius(ctx.h, dc.h, bad, None, out.h) == inv
    assert L.rsreg_cloud_radius_outlier_removal(ctx.h, dc.h, 0.1, -1, 0, 0, out.h, C.byref(kept)) == inv   # min_neighbors < 0
    assert L.rsreg_cloud_normals_radius(ctx.h, dc.h, 0.1, None, dc.h) == inv                               # out == in
    assert L.rsreg_cloud_normals_radius(ctx.h, dc.h, 0.1, None, None) == inv
    assert L.rsreg_cloud_radius_outlier_removal(ctx.h, dc.h, 0.1, 2, 0, 0, None, C.byref(kept)) == inv
    assert L.rsreg_cloud_radius_count(ctx.h, dc.h, 0.1, None) == inv
    other = api.Context(0)
    foreign_in, foreign_out = api.DeviceCloud(K.cloud(xyz), ctx=other), api.DeviceCloud(ctx=other)
    assert L.rsreg_cloud_radius_count(ctx.h, foreign_in.h, 0.1, counts.ctypes.data) == inv                 # a cloud of another context
    assert L.rsreg_cloud_radius_outlier_removal(ctx.h, foreign_in.h, 0.1, 2, 0, 0, out.h, C.byref(kept)) == inv
    assert L.rsreg_cloud_radius_outlier_removal(ctx.h, dc.h, 0.1, 2, 0, 0, foreign_out.h, C.byref(kept)) == inv
    assert L.rsreg_cloud_normals_radius(ctx.h, foreign_in.h, 0.1, None, out.h) == inv
    assert L.rsreg_cloud_normals_radius(ctx.h, dc.h, 0.1, None, foreign_out.h) == inv
    assert out.download().points.tobytes() == before and out.stamp == stamp and len(dc) == 40
    assert (counts == 77).all() and kept.value == 99 and len(foreign_out) == 0
    with pytest.raises(lib.RsregError) as e:
        dc.normals_radius(0.0)
    assert e.value.status == inv
    with pytest.raises(lib.RsregError) as e:
        dc.radius_outlier_removal(0.1, -1)
    assert e.value.status == inv
    ne = api.NormalEstimation()
    ne.setInputCloud(dc)
    ne.setKSearch(10)
    ne.setRadiusSearch(0.1)
    with pytest.raises(lib.RsregError, match="both"):
        ne.compute()
    lib.check(L.rsreg_cloud_normals_radius(ctx.h, dc.h, 0.3, None, out.h), ctx.h)                          # ... and the call that is right
    assert out.stamp[1] != stamp[1] and out.info()[:2] == (40, 32)
    assert L.rsreg_version() == 4


def test_adaptors(api, ctx, tmp_path):
    """tests/cpp/radius_runner.cpp gives the bytes of the Python device path, from host clouds and from device clouds; so do
    api.RadiusOutlierRemoval and api.NormalEstimation on a host cloud."""
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "radius_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "radius_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    fr = K.input_cloud("frame_raw")
    vp = (0.3, -0.2, 5.0)
    dc = api.DeviceCloud(fr, ctx=ctx)
    want_kept, n_kept = dc.radius_outlier_removal(0.03, 10)
    want_kept = want_kept.download()
    want = dc.normals_radius_cloud(0.03, vp).download_normals()
    assert want_kept.points.tobytes() == _records(fr.points, R.ror_keep(_ref_counts("frame_raw", 0.03), 10))
    ror = api.RadiusOutlierRemoval()
    ror.setInputCloud(fr)                                    # a host cloud: through a temporary DeviceCloud
    ror.setRadiusSearch(0.03)
    ror.setMinNeighborsInRadius(10)
    host_kept = ror.filter()
    assert host_kept.points.tobytes() == want_kept.points.tobytes() and ror.n_kept == n_kept == len(host_kept)
    assert (host_kept.width, host_kept.height, host_kept.is_dense) == (want_kept.width, want_kept.height, want_kept.is_dense)
    ne = api.NormalEstimation()
    ne.setInputCloud(fr)
    ne.setRadiusSearch(0.03)
    ne.setViewPoint(*vp)
    host = ne.compute()
    assert host.points.tobytes() == want.points.tobytes()
    assert (host.width, host.height, host.is_dense) == (fr.width, fr.height, False) == (want.width, want.height, want.is_dense)
    fr.points.tofile(str(tmp_path / "in.bin"))
    names = ["ror_host.bin", "ror_dev.bin", "n_host.bin", "n_dev.bin"]
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(fr.width), str(fr.height), "0.03", "10", "0", "0", "0.3", "-0.2", "5"] +
                       [str(tmp_path / f) for f in names], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    vals = dict(l.split() for l in r.stdout.strip().splitlines())
    for f in names[:2]:
        assert open(str(tmp_path / f), "rb").read() == want_kept.points.tobytes()
    for f in names[2:]:
        assert open(str(tmp_path / f), "rb").read() == want.points.tobytes()
    assert int(vals["ror_size"]) == int(vals["ror_size_device"]) == int(vals["ror_kept"]) == int(vals["ror_width"]) == n_kept
    assert vals["ror_height"] == "1" and vals["ror_dense"] == vals["ror_dense_device"] == "0"
    assert int(vals["size"]) == int(vals["size_device"]) == len(fr) and int(vals["width"]) == fr.width and int(vals["height"]) == fr.height
    assert vals["dense"] == vals["dense_device"] == "0" and float(vals["radius"]) == 0.03
