"""The three exact searches over the point grid of csrc/pointgrid.hpp -- knn_walk (rsreg_cloud_knn, rsreg_cloud_knn_mean_distance),
radius_walk (rsreg_cloud_radius_count, rsreg_cloud_normals_radius) and the fitness walk (getFitnessScore) -- on the thin, far,
piled-up and cell-aligned scenes of tests/pointgrid_cases.py, where the grid picks its cell by another rule than the bisection, where
the rounding of a coordinate is a sizeable part of a cell, and where the answer lies across a face, an edge or a corner of the query's
cell.  tests/test_pointgrid_layout_cpu.py holds the layout and the bound of these scenes on the CPU.

Every search claims the answer of a float32 brute force, bit for bit, and that is what is asserted, on EVERY record of every scene:
  * knn(k), k in 2, 10, 64: indices and d2 EQUAL to normals_ref.knn(xyz, k, "brute") -- one brute force at k = 65 per scene; its
    first k columns are the reference at k (ascending by (d2, index): a prefix of the order) -- rows of non-finite records included;
  * knn_mean_distance(mean_k), mean_k in 1, 50, 64: EQUAL to sor_ref.knn_mean_distance(xyz, mean_k, "brute") -- from the same brute
    force's mean_k + 1 smallest d2, by sor_ref's own sum (held against the call itself on line_x and one_point_pile);
  * radius_count(r): EQUAL to a plain float32 brute force, d2 < r2_f32(r) strictly, the record itself included; the radii are picked
    per scene from the layout (pointgrid_cases.radii: the cell stays above the radius, the radius becomes the cell, two cells per axis,
    and on far_lattice and the tie sites a radius whose float32 square IS a distance that occurs, and the float32 next above it);
  * normals_radius on cell_sites and far_box: NaN in exactly the rows with fewer than three neighbours, as the counts say;
  * the fitness score with the scene as the target and pointgrid_cases.fitness_source as the source, after an alignment with the
    reference parameters and a 1 mm gate, from the library's own transformed positions: the count exact at max_range = DBL_MAX, a
    value between two occurring distances, and 0; the score bit-equal on far_lattice (every d2 a multiple of 2^-22, the sum exact:
    asserted) and elsewhere within (n - 1) * 2^-53 * score: what any order of adding n non-negative doubles can differ by.
All of it on ONE context, the consumers interleaved (they share ctx->knn and its zero-after-use count buffer), a scene of few cells
after a scene of many and the other way round; then the knn rows of cell_sites and far_box from a fresh context: the same bytes.
"""
import functools
import sys
import time

import numpy as np
import pytest

import fitness_ref as F
import normals_ref as N
import pointgrid_cases as K
import pointgrid_layout as G
import radius_cases
import radius_ref as R
import sor_ref as S

DBL_MAX = sys.float_info.max
GATE = 1e-3
# a scene of few cells after a scene of many
ORDER = ["line_x", "far_lattice", "slab", "one_point_pile", "cell_sites", "one_point_pile_origin", "line_y", "holes",
         "cluster_and_outliers", "far_box", "line_z", "cell_sites_500"]
assert sorted(ORDER) == sorted(K.SCENES)
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
    print("\npoint-grid searches: %.1f s from the first context to the last test" % (time.perf_counter() - t0))


@functools.lru_cache(maxsize=None)
def _brute(name):
    """(idx, d2) of normals_ref.knn at k = min(65, finite records), brute force."""
    return N.knn(K.scene(name), min(65, K.finite_count(name)), method="brute")


def _want_mean(name, mean_k):
    xyz = K.scene(name)
    fin = S.finite_rows(xyz)
    out = np.zeros(len(xyz), np.float32)
    out[fin] = S._mean_of_sorted(_brute(name)[1][fin][:, :mean_k + 1], mean_k)
    return out


@functools.lru_cache(maxsize=None)
def _want_counts(name):
    """{radius: uint32 counts} by a plain float32 brute force: d2 < r2_f32(r), strictly, the record itself included; and
    {radius: how many pairs lie AT r2}."""
    xyz = K.scene(name)
    fin = np.flatnonzero(S.finite_rows(xyz))
    t = xyz[fin]
    radii = [r for _, r in K.radii(name)]
    counts = {r: np.zeros(len(xyz), np.uint32) for r in radii}
    at = {r: 0 for r in radii}
    for s in range(0, len(t), 256):
        d = F.d2_f32(t[s:s + 256, None, :], t[None, :, :])
        for r in radii:
            counts[r][fin[s:s + 256]] = (d < R.r2_f32(r)).sum(axis=1)
            at[r] += int((d == R.r2_f32(r)).sum())
    return counts, at


def _cloud(xyz):
    from rsreg_amd import POINT_DTYPE, PointCloud
    pts = np.zeros(len(xyz), POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["w"] = 1.0
    return PointCloud(pts, width=len(xyz), height=1, is_dense=False)


def _ks(name):
    """2, 10, 64 -- the largest that fits where a scene has fewer finite records."""
    nfin = K.finite_count(name)
    return sorted({min(k, nfin) for k in (2, 10, 64)})


def _mean_ks(name):
    nfin = K.finite_count(name)
    return sorted({min(k, nfin - 1) for k in (1, 50, 64)})


# ------------------------------------------------------------------------------------------------ k-NN, mean distance, radius
@pytest.mark.parametrize("name", ORDER)
def test_searches_equal_the_brute_force(api, ctx, name):
    xyz = K.scene(name)
    fin = S.finite_rows(xyz)
    lay = G.layout_of(xyz, "knn")
    ref_idx, ref_d2 = _brute(name)
    want_counts, at = _want_counts(name)
    dc = api.DeviceCloud(radius_cases.cloud(xyz), ctx=ctx)
    radii = list(K.radii(name))
    print("%s: %d records, %d finite, k-NN grid %d x %d x %d (%s)" % (name, len(xyz), int(fin.sum()), *lay.dims, lay.branch))
    wrong = []
    # the consumers take turns: every call builds its own index in ctx->knn
    turns = max(len(_ks(name)), len(_mean_ks(name)), len(radii))
    for turn in range(turns):
        if turn < len(_ks(name)):
            k = _ks(name)[turn]
            t0 = time.perf_counter()
            idx, d2 = dc.knn(k)
            dt = time.perf_counter() - t0
            bad_i, bad_d = int((idx != ref_idx[:, :k]).any(axis=1).sum()), int((d2 != ref_d2[:, :k]).any(axis=1).sum())
            ties = float((ref_d2[fin][:, 1:k] == ref_d2[fin][:, :k - 1]).mean()) if k > 1 else 0.0
            print("  knn(%d): %.3f s, rows with a wrong index %d, with a wrong d2 %d, share of ties %.3f" % (k, dt, bad_i, bad_d, ties))
            assert idx.dtype == np.int32 and d2.dtype == np.float32 and idx.shape == d2.shape == (len(xyz), k)
            if bad_i or bad_d:
                wrong.append("knn(%d)" % k)
            if (idx[~fin] != -1).any() or (d2[~fin] != 0).any():
                wrong.append("knn(%d) non-finite rows" % k)
        if turn < len(_mean_ks(name)):
            mk = _mean_ks(name)[turn]
            t0 = time.perf_counter()
            got = dc.knn_mean_distance(mk)
            dt = time.perf_counter() - t0
            want = _want_mean(name, mk)
            if name in ("one_point_pile", "line_x"):
                np.testing.assert_array_equal(want, S.knn_mean_distance(xyz, mk, method="brute"))
            bad = int((got != want).sum())
            print("  knn_mean_distance(%d): %.3f s, records that differ %d" % (mk, dt, bad))
            if bad or (got[~fin] != 0).any():
                wrong.append("knn_mean_distance(%d)" % mk)
        if turn < len(radii):
            what, r = radii[turn]
            t0 = time.perf_counter()
            got = dc.radius_count(r)
            dt = time.perf_counter() - t0
            want = want_counts[r]
            bad = int((got != want).sum())
            print("  radius_count(%s = %.9g): %.3f s, counts %d .. %d, pairs AT r2 %d, records that differ %d" %
                  (what, r, dt, want[fin].min(), want[fin].max(), at[r], bad))
            if bad:
                wrong.append("radius_count(%s)" % what)
            if what == "big":
                assert (want[fin] == fin.sum()).all()
            if what == "at":                                 # the distance occurs, and is not counted; just above, it is
                above = want_counts[radii[turn + 1][1]]
                assert at[r] > 0 and int(above.sum()) - int(want.sum()) == at[r] and radii[turn + 1][0] == "above"
    assert not wrong, (name, wrong)
    for s in K.sites(name):                                  # (what the sites are for, spelled out: the record across the face)
        if s.m + 1 in _ks(name):
            assert ref_idx[s.query, s.m] == s.true


@pytest.mark.parametrize("name,what", [("cell_sites", "at"), ("far_box", "cell"), ("cell_sites", "above")])
def test_normals_radius_nan_pattern(api, ctx, name, what):
    xyz = K.scene(name)
    r = dict(K.radii(name))[what]
    counts = _want_counts(name)[0][r]
    dc = api.DeviceCloud(radius_cases.cloud(xyz), ctx=ctx)
    got = dc.normals_radius(r)
    nan = np.isnan(got)
    print("normals_radius %s (%s = %.9g): %d of %d records with fewer than three neighbours" % (name, what, r, int((counts < 3).sum()), len(xyz)))
    assert got.shape == (len(xyz), 4)
    assert (nan.all(axis=1) == (counts < 3)).all() and (nan.any(axis=1) == nan.all(axis=1)).all()
    assert 0 < (counts < 3).sum() < len(xyz)
    np.testing.assert_array_equal(dc.radius_count(r), counts)    # ... and the counts after it, on the same index buffers


# ------------------------------------------------------------------------------------------------ the fitness score
def _xyz(pc):
    p = pc.points
    return np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float32)


@pytest.mark.parametrize("name", ORDER)
def test_fitness_score_with_the_scene_as_target(api, ctx, name):
    tgt, src = K.scene(name), K.fitness_source(name)
    icp = api.IterativeClosestPoint(ctx)
    icp.params = api.icp_params(reference=True, max_correspondence_distance=GATE)
    icp.setInputSource(_cloud(src))
    icp.setInputTarget(_cloud(tgt))
    icp.align()
    T = icp.getFinalTransformation()
    pos = _xyz(api.transformPointCloud(_cloud(src), T, ctx=ctx))
    valid = F.finite_rows(src)
    assert len(pos) * len(tgt) <= F._BRUTE                   # (fitness_ref.fitness takes the brute force)
    d = F.nearest_d2_brute(pos, tgt)
    occurring = np.unique(d[valid & np.isfinite(d)].astype(np.float64))
    between = 0.5 * (occurring[len(occurring) // 2 - 1] + occurring[len(occurring) // 2])
    lay = G.layout_of(tgt, "fit")
    print("%s: fitness grid %d x %d x %d (%s), %d correspondences, identity %s, d2 %.3g .. %.3g" %
          (name, *lay.dims, lay.branch, icp.result.n_correspondences, bool((T == np.eye(4, dtype=np.float32)).all()), occurring[0], occurring[-1]))
    exact = name == "far_lattice"
    if exact:                                                # every d2 a multiple of 2^-22, and the sum of all of them below 2^53 of those
        np.testing.assert_array_equal(T, np.eye(4, dtype=np.float32))
        units = occurring * 2.0 ** 22
        assert (units == np.round(units)).all() and d[valid].astype(np.float64).sum() * 2.0 ** 22 < 2.0 ** 53
    for max_range in (DBL_MAX, between, 0.0):
        want = F.fitness(pos, tgt, max_range, valid=valid)
        got = icp.fitnessScore(max_range)
        n = want[1]
        bound = 0.0 if exact or n == 0 else (n - 1) * 2.0 ** -53 * want[0]
        print("  max_range %.6g: %d records, score %r, reference %r, |difference| %.3g, bound %.3g" %
              (max_range, got[1], got[0], want[0], abs(got[0] - want[0]), bound))
        assert got[1] == n
        assert abs(got[0] - want[0]) <= bound
    assert icp.fitnessScore(DBL_MAX)[1] == int((valid & np.isfinite(d)).sum()) and 0 < icp.fitnessScore(between)[1] < valid.sum()


# ------------------------------------------------------------------------------------------------ bytes, on a second context
@pytest.mark.parametrize("name", ["cell_sites", "far_box"])
def test_knn_bytes_from_a_fresh_context(api, ctx, name):
    cloud = radius_cases.cloud(K.scene(name))
    fresh = api.Context(0)
    for k in (10, 64):
        a_idx, a_d2 = api.DeviceCloud(cloud, ctx=ctx).knn(k)
        b_idx, b_d2 = api.DeviceCloud(cloud, ctx=fresh).knn(k)
        assert a_idx.tobytes() == b_idx.tobytes() and a_d2.tobytes() == b_d2.tobytes()
        np.testing.assert_array_equal(a_idx, _brute(name)[0][:, :k])
