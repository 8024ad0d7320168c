"""The cloud searches and what is built on them -- rsreg_cloud_knn, rsreg_cloud_knn_mean_distance / SOR, rsreg_cloud_normals,
rsreg_cloud_radius_count / normals_radius, rsreg_icp_fitness_score, rsreg_cloud_spfh / _fpfh, PassThrough -- across the float32
range, on the clouds of tests/scale_cases.py.  tests/test_scale_cpu.py establishes, on the references alone, the window in which
scaling by 2^e commutes with all of them, and names the regime of the point grid's arithmetic at every case outside it.

(a) Inside the window (WINDOW), for every base cloud: the same call at scale 2^e and at scale 1, in the same test, BYTE for byte --
    knn indices equal and d2 * 2^2e; mean distances * 2^e and the SOR keep mask; the 32-byte normal records of normals(10),
    normals(50) and normals_radius; the radius counts at r * 2^e (on `plane`: AT the lattice spacing and one ulp above it); the
    fitness count, and score * 2^2e with max_range * 2^2e; SPFH and FPFH with the scale-1 normals; the PassThrough mask on z.
    And at scale 2^e against the references themselves, by the rules of the tests of each call.
(b) Outside it (EXTREME, MIXED): the float32 brute-force references -- overflowing d2 is +inf, ties go to the lowest index.  knn
    and mean distances bit-equal, +inf rows and +inf means included; radius counts equal (at a radius drawn from the cloud and at
    1e30, whose float32 square is +inf); the fitness count exact and the score within 1e-12 relative (tests/test_plane_icp_gpu.py's
    rule); the normals through tests/test_normals_gpu.py's checker (its bounds are relative to the trace); FPFH through
    tests/test_fpfh_gpu.py's rule where every d2 is a finite normal float (at 2^62: test_scale_cpu.py) and through
    _check_fpfh_outside elsewhere: a denormal d2 puts NaNs into the rows of finite records, in the reference's places, and the
    cloud is then not dense (test_scale_cpu.py has the table of regimes).  On the denormal cloud every d2 is 0: the answer is the
    reference's, the k lowest indices.
    The sources of a fitness score also lie far outside the target's box (FAR_TARGETS: up to 1e32 cells of a box of any size).
(c) One EXTREME case gives the same bytes from a fresh context that indexed a metre-scale cloud first.

The fitness score needs an alignment: begin() and end() with no iteration between them leave the identity as the final transform,
so the score is the one of the records as they are.
"""
import numpy as np
import pytest

import fitness_ref as F
import fpfh_cases
import fpfh_ref
import normals_ref as N
import radius_cases
import radius_ref as R
import scale_cases as C
import sor_ref as S
from test_fpfh_gpu import _check_fpfh
from test_normals_gpu import _check_normals
from test_radius_gpu import _check_normals as _check_radius_normals

pytestmark = pytest.mark.gpu
GATE = 0.05                       # of the alignment's target index, in units of the cloud's scale: nothing is searched through it


@pytest.fixture(scope="module")
def api():
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    return api


@pytest.fixture(scope="module")
def ctx(api):
    return api.Context(0)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _ldexp32(a, e):
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(np.asarray(a, np.float32), int(e)).astype(np.float32)


def _xyz(pc):
    p = pc.points
    return np.stack([p["x"], p["y"], p["z"]], 1)


def _fitness(api, ctx, src, tgt, gate, ranges):
    icp = api.IterativeClosestPoint(ctx)
    icp.params = api.icp_params(reference=True, max_correspondence_distance=gate)
    icp.setInputSource(radius_cases.cloud(src, seed=1))
    icp.setInputTarget(radius_cases.cloud(tgt))
    icp.begin()
    icp.end()
    np.testing.assert_array_equal(icp.getFinalTransformation(), np.eye(4, dtype=np.float32))
    return [icp.fitnessScore(r) for r in ranges]


def _sor_mask(api, dc, cloud, mean_k):
    f = api.StatisticalOutlierRemoval()
    f.setInputCloud(dc)
    f.setMeanK(mean_k)
    f.setStddevMulThresh(C.STD_MUL)
    out = f.filter()
    kept = out.download().points
    out.close()
    tags = cloud.points["rgba"].astype(np.uint64) << np.uint64(32) | cloud.points["w"].view(np.uint32).astype(np.uint64)
    assert len(np.unique(tags)) == len(tags)
    got = kept["rgba"].astype(np.uint64) << np.uint64(32) | kept["w"].view(np.uint32).astype(np.uint64)
    mask = np.isin(tags, got)
    assert mask.sum() == len(kept) and (got == tags[mask]).all()          # the kept records, in their order
    return mask


def _pass_mask(api, dc, lo, hi):
    f = api.PassThrough()
    f.setInputCloud(dc)
    f.setFilterFieldName("z")
    f.setFilterLimits(float(lo), float(hi))
    f.setKeepOrganized(True)
    out = f.filter()
    mask = S.finite_rows(_xyz(out.download()))
    out.close()
    return mask


def _fpfh_normals(name, four):
    """(n, 3) float32 normals for the FPFH calls from normals(10)'s output, the records of fpfh_cases.holes made non-finite."""
    nrm = np.ascontiguousarray(four[:, :3]).copy()
    bad = C.bad_normals(name)
    nrm[bad[:20]] = np.nan
    nrm[bad[20:], 2] = np.inf
    return nrm


def _window_outputs(api, ctx, name, e, nrm=None):
    """Every output of (a) for base cloud `name` at scale 2^e; nrm: the scale-1 normals of the FPFH calls (None: made here)."""
    xyz = C.scaled(C.base(name), e)
    cloud = radius_cases.cloud(xyz)
    dc = api.DeviceCloud(cloud, ctx=ctx)
    out = {"xyz": xyz, "cloud": cloud}
    out["knn"] = {k: dc.knn(k) for k in C.KS}
    out["mean"] = {k: dc.knn_mean_distance(k) for k in C.KS}
    out["sor"] = _sor_mask(api, dc, cloud, 10)
    out["normals"] = {}
    for k in C.NORMAL_KS:
        nc = dc.normals_cloud(k)
        out["normals"][k] = nc.download_normals().points
        nc.close()
    out["counts"], out["normals_radius"] = {}, {}
    for r in C.radii(name):
        re_ = C.radius_at(r, e)
        out["counts"][r] = dc.radius_count(re_)
        nc = dc.normals_radius_cloud(re_)
        out["normals_radius"][r] = nc.download_normals().points
        nc.close()
    between = float(np.ldexp(C.fitness_between(name), 2 * e))
    out["ranges"] = (F.DBL_MAX, between)
    out["src"] = C.scaled(C.jittered(C.base(name)), e)
    out["fitness"] = _fitness(api, ctx, out["src"], xyz, float(np.ldexp(GATE, e)), out["ranges"])
    rec = out["normals"][10]
    four = np.stack([rec["normal_x"], rec["normal_y"], rec["normal_z"], rec["curvature"]], axis=1)
    out["nrm"] = _fpfh_normals(name, four) if nrm is None else nrm
    out["spfh"] = dc.spfh(out["nrm"], 10)
    out["fpfh"] = dc.fpfh(out["nrm"], 10)
    lo, hi = C.pass_limits(name)
    out["limits"] = (_ldexp32(lo, e), _ldexp32(hi, e))
    out["pass"] = _pass_mask(api, dc, *out["limits"])
    dc.close()
    return out


_AT_ONE = {}


def _at_one(api, ctx, name):
    if name not in _AT_ONE:
        _AT_ONE[name] = _window_outputs(api, ctx, name, 0)
    return _AT_ONE[name]


def _four(rec):
    return np.stack([rec["normal_x"], rec["normal_y"], rec["normal_z"], rec["curvature"]], axis=1)


def _against_references(name, e, got):
    """The outputs of _window_outputs against the references at scale 2^e, by the rules of each call's own tests."""
    xyz, cloud = got["xyz"], got["cloud"]
    fin = S.finite_rows(xyz)
    b = C.brute(name, e)
    for k in C.KS:
        idx, d2 = got["knn"][k]
        assert _bits(idx) == _bits(b.idx[:, :k]) and _bits(d2) == _bits(b.d2[:, :k]), (name, e, k)
        assert _bits(got["mean"][k]) == _bits(C.mean_ref(xyz, b, k)), (name, e, k)
    m10 = C.mean_ref(xyz, b, 10)
    assert (got["sor"] == S.sor_keep(xyz, m10, S.sor_stats(xyz, m10, C.STD_MUL)[3])).all()
    for k in C.NORMAL_KS:
        ref = N.normals(xyz, k, knn_result=C.knn_ref(b, k))
        _check_normals(_four(got["normals"][k]), cloud, ref, (0.0, 0.0, 0.0), name in ("uniform", "sphere"), "%s*2^%d k=%d" % (name, e, k))
    for r in C.radii(name):
        want = C.counts_brute(xyz, C.radius_at(r, e))
        np.testing.assert_array_equal(got["counts"][r], want)
        ref = R.normals(xyz, C.radius_at(r, e))
        assert (ref.m == want).all()
        if (want >= 3).any():
            _check_radius_normals(_four(got["normals_radius"][r]), cloud, ref, (0.0, 0.0, 0.0), False, "%s*2^%d r=%.6g" % (name, e, C.radius_at(r, e)))
        else:                                                 # (plane, AT the lattice spacing: every record alone)
            assert np.isnan(_four(got["normals_radius"][r])).all()
    for r, (score, count) in zip(got["ranges"], got["fitness"]):
        want = F.fitness(got["src"], xyz, r, valid=F.finite_rows(got["src"]))
        assert count == want[1] and abs(score - want[0]) <= 1e-12 * want[0], (name, e, r, (score, count), want)
    ref = fpfh_ref.fpfh(xyz, got["nrm"], 10, knn_result=C.knn_ref(b, 10))
    _check_fpfh(got["fpfh"], ref, "fpfh %s*2^%d" % (name, e))
    np.testing.assert_array_equal(got["spfh"][~ref.fragile], ref.spfh[~ref.fragile])
    assert (got["pass"] == S.passthrough_keep(xyz, 2, *got["limits"])).all()
    assert (got["pass"][~fin] == 0).all()


# ------------------------------------------------------------------------------------------------ (a) inside the window: bytes
@pytest.mark.parametrize("name", C.BASES)
def test_scale_one_against_the_references(api, ctx, name):
    _against_references(name, 0, _at_one(api, ctx, name))


@pytest.mark.parametrize("e", C.WINDOW)
@pytest.mark.parametrize("name", C.BASES)
def test_window_gives_the_bytes_of_scale_one(api, ctx, name, e):
    one = _at_one(api, ctx, name)
    got = _window_outputs(api, ctx, name, e, nrm=one["nrm"])
    for k in C.KS:
        assert _bits(got["knn"][k][0]) == _bits(one["knn"][k][0]), (name, e, k)
        assert _bits(got["knn"][k][1]) == _bits(_ldexp32(one["knn"][k][1], 2 * e)), (name, e, k)
        assert _bits(got["mean"][k]) == _bits(_ldexp32(one["mean"][k], e)), (name, e, k)
    assert (got["sor"] == one["sor"]).all() and 0 < (~got["sor"]).sum() < len(got["sor"])
    for k in C.NORMAL_KS:
        assert _bits(got["normals"][k]) == _bits(one["normals"][k]), (name, e, k)
    for r in C.radii(name):
        assert _bits(got["counts"][r]) == _bits(one["counts"][r]), (name, e, r)
        assert _bits(got["normals_radius"][r]) == _bits(one["normals_radius"][r]), (name, e, r)
    for (score, count), (score1, count1) in zip(got["fitness"], one["fitness"]):
        assert count == count1 and score == float(np.ldexp(score1, 2 * e)), (name, e, (score, count), (score1, count1))
    assert 0 < one["fitness"][1][1] < one["fitness"][0][1]
    assert _bits(got["spfh"]) == _bits(one["spfh"]) and _bits(got["fpfh"]) == _bits(one["fpfh"]), (name, e)
    assert (got["pass"] == one["pass"]).all()
    _against_references(name, e, got)


# ------------------------------------------------------------------------------------------------ (b) outside the window: the references
def _check_fpfh_outside(got, spfh, ref, label):
    """tests/test_fpfh_gpu.py's rule where a d2 among the ten nearest is a denormal or +inf.  A denormal d2 gives w = 1 / d2 = +inf
    and 0 * inf = NaN in a finite record's row (include/rsreg.h says so); a +inf d2 gives w = 0.  NaNs stand in exactly the
    reference's places on every record -- with w = +inf every block's sum is a NaN, whatever the bins: a neighbour's SPFH block holds
    a zero bin -- and their sign and payload are not compared; every other float is bit-equal on the records that are not fragile
    and have no fragile neighbour; the rows of non-finite records are the quiet NaN 0x7fc00000; blocks sum to 100 or are zero on the
    rows without a NaN whose d2 are all finite normal floats (or 0)."""
    want_nan = np.isnan(ref.fpfh)
    ok = ~ref.fragile_nb & ~ref.nan_rows
    differ = (got.view(np.uint32) != ref.fpfh.view(np.uint32)) & ~want_nan
    bad = np.flatnonzero(differ[ok].any(axis=1))
    print("%s: records %d, fragile or fragile neighbour %d, rows with a NaN %d (of them non-finite records or normals %d), all-zero rows %d, rows that differ %d" %
          (label, len(got), int(ref.fragile_nb.sum()), int(want_nan.any(axis=1).sum()), int(ref.nan_rows.sum()), int((ref.fpfh == 0).all(axis=1).sum()), len(bad)))
    assert (np.isnan(got) == want_nan).all(), np.flatnonzero((np.isnan(got) != want_nan).any(axis=1))[:8]
    assert len(bad) == 0, (np.flatnonzero(ok)[bad[:4]], got[ok][bad[:4]], ref.fpfh[ok][bad[:4]])
    assert (got.view(np.uint32)[ref.nan_rows] == 0x7fc00000).all()
    np.testing.assert_array_equal(spfh[~ref.fragile], ref.spfh[~ref.fragile])
    sound = ~want_nan.any(axis=1) & (np.isfinite(ref.d2) & ((ref.d2 == 0) | (ref.d2 >= C.FLT_MIN))).all(axis=1)
    assert fpfh_ref.blocks_ok(got[sound]).all()


def _outside_outputs(api, ctx, dc, xyz, cloud, case):
    out = {"xyz": xyz, "cloud": cloud}
    out["knn"] = {k: dc.knn(k) for k in C.KS}
    out["mean"] = {k: dc.knn_mean_distance(k) for k in C.KS}
    out["normals"] = {k: dc.normals(k) for k in C.NORMAL_KS}
    out["radii"] = (C.outside_radius(case), 1e30)
    out["counts"] = [dc.radius_count(r) for r in out["radii"]]
    out["src"] = C.jittered(xyz)
    scale = float(np.abs(xyz[S.finite_rows(xyz)]).max())
    out["ranges"] = [r for r in C.fitness_ranges(out["src"], xyz) if r is not None]
    out["fitness"] = _fitness(api, ctx, out["src"], xyz, min(GATE * scale, 1e37), out["ranges"])
    return out


@pytest.mark.parametrize("case", C.OUTSIDE, ids=C.label)
def test_outside_the_window_equals_the_references(api, ctx, case):
    xyz = C.cloud_of(case)
    cloud = radius_cases.cloud(xyz)
    dc = api.DeviceCloud(cloud, ctx=ctx)
    try:
        _outside_case(api, ctx, dc, xyz, cloud, case)
    finally:
        dc.close()


def _outside_case(api, ctx, dc, xyz, cloud, case):
    got = _outside_outputs(api, ctx, dc, xyz, cloud, case)
    fin = S.finite_rows(xyz)
    b = C.brute_of(case)
    reg = C.regime(xyz, "knn", b)
    print("%s: cell^2 in float32 %s, float32(q - origin) %s, d2: %s" % (C.label(case), reg.cell2, reg.q_minus_origin, ", ".join(reg.d2)))
    wrong = []
    for k in C.KS:
        idx, d2 = got["knn"][k]
        bad_i, bad_d = int((idx != b.idx[:, :k]).any(axis=1).sum()), int((d2.view(np.uint32) != b.d2[:, :k].view(np.uint32)).any(axis=1).sum())
        want = C.mean_ref(xyz, b, k)
        bad_m = int((got["mean"][k].view(np.uint32) != want.view(np.uint32)).sum())
        print("  k = %d: rows with a wrong index %d, with a wrong d2 %d, wrong mean distances %d; +inf in %d rows of d2, %d means" %
              (k, bad_i, bad_d, bad_m, int(np.isinf(b.d2[:, :k]).any(axis=1).sum()), int(np.isinf(want).sum())))
        if bad_i or bad_d or bad_m:
            wrong.append("k = %d" % k)
    for r, cnt in zip(got["radii"], got["counts"]):
        want = C.counts_brute(xyz, r)
        bad = int((cnt != want).sum())
        print("  radius_count(%.6g): counts %d .. %d, records that differ %d" % (r, want[fin].min(), want[fin].max(), bad))
        if bad:
            wrong.append("radius_count(%.6g)" % r)
    for r, (score, count) in zip(got["ranges"], got["fitness"]):
        want = F.fitness(got["src"], xyz, r, valid=F.finite_rows(got["src"]))
        print("  fitness(max_range %.6g): %r, reference %r" % (r, (score, count), want))
        if count != want[1] or not (score == want[0] or abs(score - want[0]) <= 1e-12 * want[0]):
            wrong.append("fitness(%.6g)" % r)
    assert not wrong, (C.label(case), wrong)
    for k in C.NORMAL_KS:
        ref = N.normals(xyz, k, knn_result=C.knn_ref(b, k))
        _check_normals(got["normals"][k], cloud, ref, (0.0, 0.0, 0.0), False, "%s k=%d" % (C.label(case), k))
    d10 = b.d2[fin][:, :10]
    name = case if isinstance(case, str) else case[0]
    nrm = _fpfh_normals(name, got["normals"][10])
    ref = fpfh_ref.fpfh(xyz, nrm, 10, knn_result=C.knn_ref(b, 10))
    if (np.isfinite(d10) & ((d10 == 0) | (d10 >= C.FLT_MIN))).all():        # every d2 a finite normal float (or 0: a copy)
        _check_fpfh(dc.fpfh(nrm, 10), ref, "fpfh %s" % C.label(case))
        np.testing.assert_array_equal(dc.spfh(nrm, 10)[~ref.fragile], ref.spfh[~ref.fragile])
    else:                                                                   # a denormal or +inf d2: 1 / d2 is +inf or 0
        _check_fpfh_outside(dc.fpfh(nrm, 10), dc.spfh(nrm, 10), ref, "fpfh %s" % C.label(case))
    if case == "denormal":                                                  # every d2 is 0: the k lowest indices, for every record
        assert (b.d2 == 0).all() and (b.idx[:, :10] == np.arange(10)).all()
        assert (got["knn"][10][0] == np.arange(10)).all() and (got["mean"][10] == 0).all()
        assert (got["counts"][0] == len(xyz)).all()


@pytest.mark.parametrize("e,dense", [(-62, False), (-70, False), (70, True), (100, True)])
def test_fpfh_cloud_is_dense_only_without_nans(api, ctx, e, dense):
    """include/rsreg.h: "is_dense 0 if any record got NaNs".  At 2^-62 and 2^-70 every d2 of the uniform box is a denormal, 1 / d2 is
    +inf and every row of every (finite) record holds NaNs: the cloud is not dense, and matching it against itself finds no valid
    row.  At 2^70 and 2^100 the weights are 0, the rows zeros: no NaN, dense.  (tests/test_scale_cpu.py has the table.)"""
    xyz = C.cloud_of(("uniform", e))
    nrm = np.ascontiguousarray(fpfh_cases.ref_normals("uniform"))
    ref = fpfh_ref.fpfh(xyz, nrm, 10, knn_result=C.knn_ref(C.brute("uniform", e), 10))
    assert not ref.nan_rows.any() and np.isnan(ref.fpfh).any() == (not dense)
    dc = api.DeviceCloud(radius_cases.cloud(xyz, is_dense=True), ctx=ctx)
    out = dc.fpfh_cloud(nrm, 10)
    try:
        rows = out.download_fpfh().points["histogram"]
        assert (np.isnan(rows) == np.isnan(ref.fpfh)).all()
        assert out.info() == (len(xyz), 132, len(xyz), 1, dense)
        found = out.feature_correspondences(out)
        if dense:
            assert (rows == 0).all(axis=1).sum() >= 1400 and len(found) == len(xyz)
        else:
            assert np.isnan(rows).any(axis=1).all() and len(found) == 0 and len(out.feature_correspondences(out, reciprocal=True)) == 0
    finally:
        out.close()
        dc.close()


@pytest.mark.parametrize("case", C.FAR_TARGETS, ids=C.label)
def test_fitness_of_sources_far_outside_the_target(api, ctx, case):
    """The queries of a fitness score are not points of the index: source records up to 1e32 cells outside a target box of 1e-21,
    1e-9, 1 and 1e12 units, against fitness_ref -- the count exact, the score within 1e-12 relative."""
    tgt, src = C.cloud_of(case), C.far_source(case)
    d = F.nearest_d2_brute(src, tgt)
    occ = np.unique(d[np.isfinite(d)].astype(np.float64))
    ranges = (F.DBL_MAX, C.fitness_ranges(src, tgt)[1], 0.5 * (occ[-3] + occ[-2]), 2.0)
    got = _fitness(api, ctx, src, tgt, float(np.ldexp(GATE, case[1])), ranges)
    wrong = []
    for r, (score, count) in zip(ranges, got):
        want = F.fitness(src, tgt, r, valid=F.finite_rows(src))
        print("%s, max_range %.6g: %r, reference %r" % (C.label(case), r, (score, count), want))
        if count != want[1] or not (score == want[0] or abs(score - want[0]) <= 1e-12 * want[0]):
            wrong.append(r)
    assert not wrong, (C.label(case), wrong)
    assert got[0][1] > len(tgt[::10])                                       # far records with a finite float distance are counted


# ------------------------------------------------------------------------------------------------ (c) bytes, on a second context
@pytest.mark.parametrize("case", [("uniform", 70), "wide_and_1e23"], ids=C.label)
def test_bytes_from_a_fresh_context(api, ctx, case):
    cloud = radius_cases.cloud(C.cloud_of(case))
    fresh = api.Context(0)
    first = api.DeviceCloud(radius_cases.cloud(C.base("sphere")), ctx=fresh)
    first.normals(50)                                                       # a metre-scale cloud indexed first
    a, bb = api.DeviceCloud(cloud, ctx=ctx), api.DeviceCloud(cloud, ctx=fresh)
    for k in (10, 64):
        (ai, ad), (bi, bd) = a.knn(k), bb.knn(k)
        assert _bits(ai) == _bits(bi) and _bits(ad) == _bits(bd)
        assert _bits(a.knn_mean_distance(k)) == _bits(bb.knn_mean_distance(k))
    assert _bits(a.normals(10)) == _bits(bb.normals(10))
    r = C.outside_radius(case)
    assert _bits(a.radius_count(r)) == _bits(bb.radius_count(r))
    np.testing.assert_array_equal(a.knn(10)[0], C.brute_of(case).idx[:, :10])
