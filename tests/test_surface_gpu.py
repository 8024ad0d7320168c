"""setSearchSurface on the GPU -- rsreg_cloud_radius_count_surface, rsreg_cloud_normals_radius_surface,
rsreg_cloud_fpfh_radius_surface, rsreg_cloud_spfh_radius_surface, the Python and C++ adaptors -- against tests/surface_ref.py on the
cases of tests/surface_cases.py.

The counts are EQUAL to the reference for every query.  The needed set and its size are the reference's; the SPFH rows are BIT-EQUAL
on every needed surface record that is not fragile and zero on every record that is not needed.  The FPFH rows go by the rule of
tests/test_fpfh_radius_gpu.py::_check (derived there): on every query without a fragile surface neighbour the same NaN mask, every
value within ONE float32 step, and at most 1 value in 10 000 that differs at all.  The normals go by the bounds of
tests/test_radius_gpu.py::_check_normals (that function is called), with m the surface count.  With queries == surface every call
gives the BYTES of the in-cloud call.  The conditions on the inputs are checked on the reference alone in
tests/test_surface_cpu.py and again here.
"""
import os
import subprocess
import types

import numpy as np
import pytest

import fpfh_cases as K
import fpfh_radius_cases as C
import fpfh_radius_ref as FR
import fpfh_ref as F
import surface_cases as SC
import surface_ref as SR
from test_fpfh_radius_gpu import _cloud, _differing, _normal_cloud, _records
from test_radius_gpu import _check_normals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
QNAN = 0x7fc00000


@pytest.fixture(scope="module")
def api():
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    return api


@pytest.fixture(scope="module")
def ctx(api):
    return api.Context(0)


_DEV = {}


def _surface(api, ctx, name):
    """(DeviceCloud of the surface, DeviceCloud of its normals) of a case of fpfh_radius_cases, uploaded once"""
    if name not in _DEV:
        xyz, nrm, _ = C.case(name)
        _DEV[name] = (api.DeviceCloud(_cloud(xyz), ctx=ctx), api.DeviceCloud(_normal_cloud(api, nrm), ctx=ctx))
    return _DEV[name]


def _queries(api, ctx, q, **kw):
    return api.DeviceCloud(_cloud(np.asarray(q, np.float32).reshape(-1, 3), seed=9, **kw), ctx=ctx)


def _normals4(dev):
    rec = dev.download_normals().points
    return np.stack([rec["normal_x"], rec["normal_y"], rec["normal_z"], rec["curvature"]], axis=1)


def _check_fpfh(got, ref, label):
    """The FPFH rule of tests/test_fpfh_radius_gpu.py::_check on the queries; prints each figure before it asserts."""
    ok = ~ref.fragile_nb
    want = ref.fpfh
    differ = _differing(np.ascontiguousarray(got[ok]), np.ascontiguousarray(want[ok]))
    both = ok[:, None] & ~np.isnan(got) & ~np.isnan(want)
    steps = FR.ulp_apart(np.ascontiguousarray(got[both]), np.ascontiguousarray(want[both]))
    print("%s: queries %d, with a fragile neighbour %d, FPFH values that differ %d of %d, largest distance %d steps"
          % (label, len(want), int((~ok).sum()), differ, int(ok.sum()) * 33, int(steps.max()) if len(steps) else 0))
    assert (~ok).mean() <= SC.FRAGILE_NB_CAP
    assert (np.isnan(got[ok]) == np.isnan(want[ok])).all()
    assert (steps <= 1).all()
    assert differ <= SC.DIFFER_CAP * int(ok.sum()) * 33
    assert (got[ref.nan_rows].view(np.uint32) == QNAN).all()
    assert F.blocks_ok(got[~np.isnan(got).any(axis=1)]).all()


@pytest.mark.parametrize("name,pick", SC.CASES, ids=SC.IDS)
def test_equal_to_the_reference(api, ctx, name, pick):
    q, s, nrm, radius = SC.case(name, pick)
    ref, refn = SC.ref(name, pick), SC.ref_normals(name, pick)
    moved = _differing(ref.fpfh, SC.ref(name, pick, "descending").fpfh)
    assert moved <= SC.DIFFER_CAP * ref.fpfh.size and (ref.needed.mean() < SC.NEEDED_CAP or (name, pick) not in SC.SUBSET)
    surface, normals = _surface(api, ctx, name)
    dq = _queries(api, ctx, q)
    # counts
    m = dq.radius_count_surface(surface, radius)
    print("%s 1/%d: queries %d, m %d .. %d, counts that differ %d" % (name, pick, len(q), ref.m.min(), ref.m.max(), int((m != ref.m).sum())))
    assert m.dtype == np.uint32 and m.shape == (len(q),)
    np.testing.assert_array_equal(m, ref.m)
    # SPFH: the needed set, its rows, zero elsewhere
    spfh, needed, m2 = dq.spfh_radius_surface(surface, normals, radius)
    out, n_spfh = dq.fpfh_radius_surface_cloud(surface, normals, radius, n_spfh=True)
    sound = ref.needed & ~ref.fragile
    print("    needed %d of %d (engine %d), fragile among them %d, SPFH rows that differ %d"
          % (int(ref.needed.sum()), len(s), n_spfh, int((ref.needed & ref.fragile).sum()), int((spfh[sound] != ref.spfh[sound]).any(axis=1).sum())))
    assert (m2 == ref.m).all() and needed.dtype == np.uint32
    assert (needed == ref.needed.astype(np.uint32)).all() and n_spfh == int(ref.needed.sum())
    assert spfh[sound].tobytes() == ref.spfh[sound].tobytes()
    assert (spfh[~ref.needed].view(np.uint32) == 0).all()
    # ... and they are the rows of the in-cloud call on the surface
    assert spfh[ref.needed].tobytes() == surface.spfh_radius(normals, radius)[ref.needed].tobytes()
    # FPFH
    got = out.download_fpfh().points["histogram"]
    assert got.shape == (len(q), 33) and got.dtype == np.float32
    _check_fpfh(got, ref, "%s 1/%d" % (name, pick))
    assert out.info() == (len(q), 132, len(q), 1, False)                          # the far queries' rows are NaN
    assert dq.fpfh_radius_surface(surface, normals, radius).tobytes() == got.tobytes()
    # normals
    nd = dq.normals_radius_surface_cloud(surface, radius)
    assert nd.info() == (len(q), 32, len(q), 1, False)
    got_n = _normals4(nd)
    _check_normals(got_n, types.SimpleNamespace(xyz=np.asarray(q)), refn, (0.0, 0.0, 0.0), True, "%s 1/%d normals" % (name, pick))
    assert (got_n[~refn.valid].view(np.uint32) == QNAN).all()
    assert dq.normals_radius_surface(surface, radius).tobytes() == got_n.tobytes()


def test_viewpoint_is_seen_from_the_query(api, ctx):
    name, pick = "sphere_0.2", 40
    q, s, nrm, radius = SC.case(name, pick)
    vp = (0.3, -0.2, 5.0)
    surface, _ = _surface(api, ctx, name)
    got = _queries(api, ctx, q).normals_radius_surface(surface, radius, viewpoint=vp)
    _check_normals(got, types.SimpleNamespace(xyz=np.asarray(q)), SC.ref_normals(name, pick, vp), vp, True, "sphere, viewpoint")
    assert (got[:, :3] != _queries(api, ctx, q).normals_radius_surface(surface, radius)[:, :3]).any()


def test_lattice_by_hand(api, ctx):
    """tests/test_surface_cpu.py::test_lattice_by_hand on the engine: 10 neighbours at r = 1.5 H, the ten AT the radius are not;
    20 at the next float above."""
    lat = K.lattice()
    surface = api.DeviceCloud(_cloud(lat), ctx=ctx)
    query = _queries(api, ctx, lat[5 * 144 + 5 * 12 + 5] + np.float32([K.H / 2, 0, 0]))
    assert query.radius_count_surface(surface, 1.5 * K.H).tolist() == [10]
    assert query.radius_count_surface(surface, float(np.nextafter(np.float32(1.5 * K.H), np.float32(1)))).tolist() == [20]


def test_a_query_on_a_surface_record(api, ctx):
    """Counted in m, skipped in the weighting: with twelve copies and nothing else in range, 33 zeros and not NaN -- and a dense
    output; a query on an ordinary record gets that record's in-cloud count."""
    xyz, nrm, radius = C.case("pile")
    surface, normals = _surface(api, ctx, "pile")
    q = np.float32([C.PILE_AT, xyz[7]])
    ref = SR.fpfh(q, xyz, nrm, radius, surface_ref=C.ref("pile"))
    dq = _queries(api, ctx, q)
    m = dq.radius_count_surface(surface, radius)
    assert m.tolist() == [13, int(C.ref("pile").m[7])] == ref.m.tolist()
    out = dq.fpfh_radius_surface_cloud(surface, normals, radius)
    got = out.download_fpfh().points["histogram"]
    assert (got[0].view(np.uint32) == 0).all() and (got[1] != 0).any() and out.info()[4] is True
    _check_fpfh(got, ref, "pile")
    assert got[1].tobytes() == surface.fpfh_radius(normals, radius)[7].tobytes()


def test_placement(api, ctx):
    """Queries just outside each face of the surface's box with neighbours inside; more than a radius outside; at 1e30 and 2^100;
    a non-finite one among them.  No fault, and the context goes on."""
    xyz, nrm, radius = C.case("uniform_0.12")
    surface, normals = _surface(api, ctx, "uniform_0.12")
    near, far = [], []
    for axis in range(3):
        for pick, sign in ((np.argmin, -1.0), (np.argmax, 1.0)):
            p = xyz[pick(xyz[:, axis])].copy()
            for dist, into in ((0.05, near), (0.2, far)):
                o = p.copy()
                o[axis] += np.float32(sign * dist)
                into.append(o)
    q = np.float32(near + far + [[1e30, 0, 0], [0, 2.0 ** 100, 0], [-1e30, -1e30, 2.0 ** 100], [np.nan, 0.5, 0.5], [0.0, np.inf, 0.5], xyz[3]])
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    assert ((q[:12] < lo) | (q[:12] > hi)).any(axis=1).all()                      # all twelve lie outside the box
    ref = SR.fpfh(q, xyz, nrm, radius, surface_ref=C.ref("uniform_0.12"))
    refn = SR.normals(q, xyz, radius)
    assert (ref.m[:6] >= 1).all() and (ref.m[6:17] == 0).all() and ref.m[17] >= 1
    dq = _queries(api, ctx, q)
    m = dq.radius_count_surface(surface, radius)
    np.testing.assert_array_equal(m, ref.m)
    out = dq.fpfh_radius_surface_cloud(surface, normals, radius)
    got = out.download_fpfh().points["histogram"]
    _check_fpfh(got, ref, "placement")
    assert (got[6:17].view(np.uint32) == QNAN).all() and not np.isnan(got[17]).any() and out.info()[4] is False
    got_n = dq.normals_radius_surface(surface, radius)
    _check_normals(got_n, types.SimpleNamespace(xyz=q), refn, (0.0, 0.0, 0.0), True, "placement normals")
    # the surface far from the origin of a tiny box: queries a box away on every side
    assert _queries(api, ctx, xyz[:5] + np.float32(7.0)).radius_count_surface(surface, radius).tolist() == [0] * 5
    assert (surface.radius_count(radius) == C.ref("uniform_0.12").m).all()        # the context goes on


@pytest.mark.parametrize("name", ["corner_0.12", "sphere_0.2", "many"])
def test_queries_equal_to_the_surface_give_the_in_cloud_bytes(api, ctx, name):
    """The same handle as queries and surface: counts, normals and FPFH are the bytes of the in-cloud calls, and every finite
    record is needed.  `many`: 66 000 records, past the 65 536 workgroups of the query loops and of the SPFH list."""
    xyz, nrm, radius = C.case(name)
    surface, normals = _surface(api, ctx, name)
    assert surface.radius_count_surface(surface, radius).tobytes() == surface.radius_count(radius).tobytes()
    assert surface.normals_radius_surface(surface, radius).tobytes() == surface.normals_radius(radius).tobytes()
    out, n_spfh = surface.fpfh_radius_surface_cloud(surface, normals, radius, n_spfh=True)
    got = out.download_fpfh().points["histogram"]
    own = np.isfinite(nrm).all(axis=1)
    assert own.all() and n_spfh == len(xyz)
    assert got.tobytes() == surface.fpfh_radius(normals, radius).tobytes()
    spfh, needed, m = surface.spfh_radius_surface(surface, normals, radius)
    want_spfh, want_m = surface.spfh_radius(normals, radius, counts=True)
    assert needed.all() and spfh.tobytes() == want_spfh.tobytes() and m.tobytes() == want_m.tobytes()


def test_own_normal_rule_is_not_here(api, ctx):
    """holes: the in-cloud call gives NaNs to a record whose own normal is not finite; as a query it has no normal."""
    xyz, nrm, radius = C.case("holes")
    surface, normals = _surface(api, ctx, "holes")
    got = surface.fpfh_radius_surface(surface, normals, radius)
    want = surface.fpfh_radius(normals, radius)
    fin = np.isfinite(xyz).all(axis=1)
    own = np.isfinite(nrm).all(axis=1)
    assert (fin & ~own).sum() == C.HOLES_BAD_NORMALS
    assert got[fin & own].tobytes() == want[fin & own].tobytes()
    assert np.isnan(want[fin & ~own]).all() and not np.isnan(got[fin & ~own]).any()
    assert (got[~fin].view(np.uint32) == QNAN).all()
    ref = SR.fpfh(xyz, xyz, nrm, radius, surface_ref=C.ref("holes"))
    _check_fpfh(got, ref, "holes on itself")


def test_the_order_of_the_queries_reaches_no_bit(api, ctx):
    name, pick = "corner_0.12", 40
    q, s, nrm, radius = SC.case(name, pick)
    surface, normals = _surface(api, ctx, name)
    perm = np.random.default_rng(4).permutation(len(q))
    a, b = _queries(api, ctx, q), _queries(api, ctx, np.asarray(q)[perm])
    assert a.radius_count_surface(surface, radius)[perm].tobytes() == b.radius_count_surface(surface, radius).tobytes()
    assert a.normals_radius_surface(surface, radius)[perm].tobytes() == b.normals_radius_surface(surface, radius).tobytes()
    assert a.fpfh_radius_surface(surface, normals, radius)[perm].tobytes() == b.fpfh_radius_surface(surface, normals, radius).tobytes()
    sa, sb = a.spfh_radius_surface(surface, normals, radius), b.spfh_radius_surface(surface, normals, radius)
    assert sa[0].tobytes() == sb[0].tobytes() and sa[1].tobytes() == sb[1].tobytes()


def test_determinism(api, ctx):
    name, pick = "corner_0.12", 40
    q, s, nrm, radius = SC.case(name, pick)
    surface, normals = _surface(api, ctx, name)
    dq = _queries(api, ctx, q)
    first = dq.fpfh_radius_surface(surface, normals, radius).tobytes()
    first_n = dq.normals_radius_surface(surface, radius).tobytes()
    assert dq.fpfh_radius_surface(surface, normals, radius).tobytes() == first          # a second call
    assert dq.normals_radius_surface(surface, radius).tobytes() == first_n
    other = api.Context(0)                                                # a fresh context that first indexed another cloud at another radius
    sx, sn, sr = C.case("sphere_0.2")
    sph = api.DeviceCloud(_cloud(sx), ctx=other)
    sph.fpfh_radius(_normal_cloud(api, sn), sr)
    there, there_q = api.DeviceCloud(_cloud(s, seed=5), ctx=other), api.DeviceCloud(_cloud(np.asarray(q), seed=6), ctx=other)
    assert there_q.fpfh_radius_surface(there, _normal_cloud(api, nrm), radius).tobytes() == first
    assert there_q.normals_radius_surface(there, radius).tobytes() == first_n


@pytest.mark.parametrize("power", [-20, 20])
def test_scaled_by_a_power_of_two(api, ctx, power):
    """Both clouds and the radius times 2^power: the bytes of scale 1 (tests/test_fpfh_radius_gpu.py gives the argument)."""
    name, pick = "corner_0.12", 40
    q, s, nrm, radius = SC.case(name, pick)
    surface, normals = _surface(api, ctx, name)
    dq = _queries(api, ctx, q)
    ss, sq = api.DeviceCloud(_cloud(np.ldexp(s, power), seed=3), ctx=ctx), _queries(api, ctx, np.ldexp(np.asarray(q), power))
    r = float(np.ldexp(radius, power))
    assert sq.radius_count_surface(ss, r).tobytes() == dq.radius_count_surface(surface, radius).tobytes()
    assert sq.fpfh_radius_surface(ss, normals, r).tobytes() == dq.fpfh_radius_surface(surface, normals, radius).tobytes()
    a, b = sq.spfh_radius_surface(ss, normals, r), dq.spfh_radius_surface(surface, normals, radius)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    got, want = sq.normals_radius_surface(ss, r), dq.normals_radius_surface(surface, radius)
    assert got[:, :3].tobytes() == want[:, :3].tobytes() and got[:, 3].tobytes() == want[:, 3].tobytes()


def test_record_layouts(api, ctx):
    """12-, 16- and 48-byte query and surface records, 12- and 32-byte normal records: the same bytes."""
    name, pick = "corner_0.05", 40
    q, s, nrm, radius = SC.case(name, pick)
    surface, normals = _surface(api, ctx, name)
    dq = _queries(api, ctx, q)
    first = dq.fpfh_radius_surface(surface, normals, radius).tobytes()
    first_n = dq.normals_radius_surface(surface, radius).tobytes()
    first_m = dq.radius_count_surface(surface, radius).tobytes()
    for qf, sf, nf in ((3, 4, 3), (4, 12, 8), (12, 3, 3), (3, 3, 8), (12, 12, 8)):
        oq = api.DeviceCloud(_records(api, np.asarray(q), qf), ctx=ctx)
        osf = api.DeviceCloud(_records(api, np.asarray(s), sf), ctx=ctx)
        on = api.DeviceCloud(_records(api, np.asarray(nrm), nf, fill=np.nan), ctx=ctx)
        assert (oq.info()[1], osf.info()[1], on.info()[1]) == (4 * qf, 4 * sf, 4 * nf)
        assert oq.radius_count_surface(osf, radius).tobytes() == first_m
        assert oq.normals_radius_surface(osf, radius).tobytes() == first_n
        assert oq.fpfh_radius_surface(osf, on, radius).tobytes() == first
    assert dq.fpfh_radius_surface(surface, np.asarray(nrm), radius).tobytes() == first      # an (n, 3) array: uploaded as 12-byte records


def test_output_metadata(api, ctx):
    """width and height are the queries'; is_dense is false exactly when a row is NaN, otherwise the queries' own."""
    name, pick = "corner_0.12", 40
    q, s, nrm, radius = SC.case(name, pick)
    surface, normals = _surface(api, ctx, name)
    assert len(q) == 57
    organized = _queries(api, ctx, q, width=19, height=3)
    assert organized.fpfh_radius_surface_cloud(surface, normals, radius).info() == (57, 132, 19, 3, False)
    assert organized.normals_radius_surface_cloud(surface, radius).info() == (57, 32, 19, 3, False)
    inner = np.asarray(q)[-7:-2]                                                  # five surface records: neighbours everywhere
    assert (SR.counts(inner, s, radius) >= 3).all()
    for dense in (True, False):
        dq = _queries(api, ctx, inner, width=5, height=1, is_dense=dense)
        out = dq.fpfh_radius_surface_cloud(surface, normals, radius)
        assert out.info() == (5, 132, 5, 1, dense) and not np.isnan(out.download_fpfh().points["histogram"]).any()
        nd = dq.normals_radius_surface_cloud(surface, radius)
        assert nd.info() == (5, 32, 5, 1, dense) and not np.isnan(_normals4(nd)).any()
    two = _queries(api, ctx, np.concatenate([inner, SC.FAR[:1]]))                 # m = 0: fewer than three for the normal too
    assert two.fpfh_radius_surface_cloud(surface, normals, radius).info()[4] is False
    assert two.normals_radius_surface_cloud(surface, radius).info()[4] is False


def test_refusals(api, ctx):
    from rsreg_amd import lib
    L = lib.lib()
    inv = lib.RSREG_ERR_INVALID_ARG
    xyz = K.uniform(40, 8)
    surface = api.DeviceCloud(_cloud(xyz), ctx=ctx)
    nd = surface.normals_cloud(10)
    dq = _queries(api, ctx, xyz[:9] + np.float32(0.01))
    out = api.DeviceCloud(_cloud(K.uniform(7, 9)), ctx=ctx)
    before, stamp = out.download().points.tobytes(), out.stamp
    host, needed, cnt = np.zeros((40, 33), np.float32), np.zeros(40, np.uint32), np.zeros(9, np.uint32)
    n = lib.C.c_uint64(77)
    nref = lib.C.byref(n)
    vp = np.zeros(3, np.float32).ctypes.data
    for radius in (0.0, -0.1, float("nan"), float("inf"), float("-inf")):
        assert L.rsreg_cloud_radius_count_surface(ctx.h, dq.h, surface.h, radius, cnt.ctypes.data) == inv
        assert L.rsreg_cloud_normals_radius_surface(ctx.h, dq.h, surface.h, radius, vp, out.h) == inv
        assert L.rsreg_cloud_fpfh_radius_surface(ctx.h, dq.h, surface.h, nd.h, radius, out.h, nref) == inv
        assert L.rsreg_cloud_spfh_radius_surface(ctx.h, dq.h, surface.h, nd.h, radius, host.ctypes.data, needed.ctypes.data, cnt.ctypes.data) == inv
    for bad_out in (dq, surface, nd):                                             # out equal to an input
        assert L.rsreg_cloud_fpfh_radius_surface(ctx.h, dq.h, surface.h, nd.h, 0.1, bad_out.h, nref) == inv
    for bad_out in (dq, surface):
        assert L.rsreg_cloud_normals_radius_surface(ctx.h, dq.h, surface.h, 0.1, vp, bad_out.h) == inv
    # a null argument
    assert L.rsreg_cloud_radius_count_surface(ctx.h, dq.h, surface.h, 0.1, None) == inv
    assert L.rsreg_cloud_radius_count_surface(ctx.h, None, surface.h, 0.1, cnt.ctypes.data) == inv
    assert L.rsreg_cloud_radius_count_surface(ctx.h, dq.h, None, 0.1, cnt.ctypes.data) == inv
    assert L.rsreg_cloud_radius_count_surface(None, dq.h, surface.h, 0.1, cnt.ctypes.data) == inv
    assert L.rsreg_cloud_normals_radius_surface(ctx.h, dq.h, surface.h, 0.1, vp, None) == inv
    assert L.rsreg_cloud_normals_radius_surface(ctx.h, None, surface.h, 0.1, vp, out.h) == inv
    assert L.rsreg_cloud_normals_radius_surface(ctx.h, dq.h, None, 0.1, vp, out.h) == inv
    assert L.rsreg_cloud_fpfh_radius_surface(ctx.h, dq.h, surface.h, nd.h, 0.1, None, nref) == inv
    assert L.rsreg_cloud_fpfh_radius_surface(ctx.h, dq.h, surface.h, None, 0.1, out.h, nref) == inv
    assert L.rsreg_cloud_fpfh_radius_surface(ctx.h, dq.h, None, nd.h, 0.1, out.h, nref) == inv
    assert L.rsreg_cloud_fpfh_radius_surface(ctx.h, None, surface.h, nd.h, 0.1, out.h, nref) == inv
    assert L.rsreg_cloud_fpfh_radius_surface(None, dq.h, surface.h, nd.h, 0.1, out.h, nref) == inv
    assert L.rsreg_cloud_spfh_radius_surface(ctx.h, dq.h, surface.h, nd.h, 0.1, None, needed.ctypes.data, cnt.ctypes.data) == inv
    assert L.rsreg_cloud_spfh_radius_surface(ctx.h, dq.h, surface.h, None, 0.1, host.ctypes.data, None, None) == inv
    # normals whose size is not the surface's (the queries' size is not it)
    short = api.DeviceCloud(_normal_cloud(api, C._unit(39, 1)), ctx=ctx)
    qsize = api.DeviceCloud(_normal_cloud(api, C._unit(9, 1)), ctx=ctx)
    for bad in (short, qsize):
        assert L.rsreg_cloud_fpfh_radius_surface(ctx.h, dq.h, surface.h, bad.h, 0.1, out.h, nref) == inv
        assert L.rsreg_cloud_spfh_radius_surface(ctx.h, dq.h, surface.h, bad.h, 0.1, host.ctypes.data, needed.ctypes.data, cnt.ctypes.data) == inv
    # a cloud of another context, each in turn
    other = api.Context(0)
    fq, fs = api.DeviceCloud(_cloud(xyz[:9]), ctx=other), api.DeviceCloud(_cloud(xyz), ctx=other)
    fn, fo = api.DeviceCloud(_normal_cloud(api, C._unit(40, 2)), ctx=other), api.DeviceCloud(ctx=other)
    for a, b, c, d in ((fq, surface, nd, out), (dq, fs, nd, out), (dq, surface, fn, out), (dq, surface, nd, fo)):
        assert L.rsreg_cloud_fpfh_radius_surface(ctx.h, a.h, b.h, c.h, 0.1, d.h, nref) == inv
    for a, b, d in ((fq, surface, out), (dq, fs, out), (dq, surface, fo)):
        assert L.rsreg_cloud_normals_radius_surface(ctx.h, a.h, b.h, 0.1, vp, d.h) == inv
    assert L.rsreg_cloud_radius_count_surface(ctx.h, fq.h, surface.h, 0.1, cnt.ctypes.data) == inv
    assert L.rsreg_cloud_radius_count_surface(ctx.h, dq.h, fs.h, 0.1, cnt.ctypes.data) == inv
    assert out.download().points.tobytes() == before and out.stamp == stamp
    assert (host == 0).all() and (needed == 0).all() and (cnt == 0).all() and n.value == 77
    with pytest.raises(lib.RsregError) as e:
        dq.fpfh_radius_surface(surface, nd, 0.0)
    assert e.value.status == inv
    lib.check(L.rsreg_cloud_fpfh_radius_surface(ctx.h, dq.h, surface.h, nd.h, 0.3, out.h, nref), ctx.h)      # ... and the next valid call works
    assert out.stamp == (stamp[0], stamp[1] + 1) and out.info()[:4] == (9, 132, 9, 1) and 0 < n.value <= 40
    lib.check(L.rsreg_cloud_fpfh_radius_surface(ctx.h, dq.h, surface.h, nd.h, 0.3, out.h, None), ctx.h)      # n_spfh may be NULL
    assert L.rsreg_version() == 4


def test_empty_and_degenerate_inputs(api, ctx):
    xyz, nrm, radius = C.case("corner_0.05")
    surface, normals = _surface(api, ctx, "corner_0.05")
    empty = api.DeviceCloud(_cloud(np.zeros((0, 3), np.float32)), ctx=ctx)
    no_normals = api.DeviceCloud(_normal_cloud(api, np.zeros((0, 3), np.float32)), ctx=ctx)
    # empty queries: an empty out of the right stride, nothing needed
    out, n_spfh = empty.fpfh_radius_surface_cloud(surface, normals, radius, n_spfh=True)
    assert out.info()[:2] == (0, 132) and n_spfh == 0 and len(out.download_fpfh().points) == 0
    assert empty.normals_radius_surface_cloud(surface, radius).info()[:2] == (0, 32)
    assert len(empty.radius_count_surface(surface, radius)) == 0
    spfh, needed, m = empty.spfh_radius_surface(surface, normals, radius)
    assert spfh.shape == (len(xyz), 33) and (spfh.view(np.uint32) == 0).all() and not needed.any() and len(m) == 0
    # an empty surface, and a surface without a finite record: every count 0, every row NaN, nothing needed
    bad = np.full((70, 3), np.nan, np.float32)
    bad[::3, 1] = np.inf
    q = np.asarray(SC.queries("corner_0.05", 40))
    dq = _queries(api, ctx, q, width=19, height=3)
    for surf, snrm, ns in ((empty, no_normals, 0), (api.DeviceCloud(_cloud(bad), ctx=ctx), api.DeviceCloud(_normal_cloud(api, C._unit(70, 4)), ctx=ctx), 70)):
        assert (dq.radius_count_surface(surf, 0.5) == 0).all()
        out, n_spfh = dq.fpfh_radius_surface_cloud(surf, snrm, 0.5, n_spfh=True)
        assert out.info() == (57, 132, 19, 3, False) and n_spfh == 0
        assert (out.download_fpfh().points["histogram"].view(np.uint32) == QNAN).all()
        nd = dq.normals_radius_surface_cloud(surf, 0.5)
        assert nd.info() == (57, 32, 19, 3, False)
        rec = nd.download_normals().points
        assert (_normals4(nd).view(np.uint32) == QNAN).all() and (rec.view(np.uint32).reshape(57, 8)[:, [3, 5, 6, 7]] == 0).all()
        spfh, needed, m = dq.spfh_radius_surface(surf, snrm, 0.5)
        assert spfh.shape == (ns, 33) and (spfh.view(np.uint32) == 0).all() and not needed.any() and (m == 0).all()
    assert (dq.radius_count_surface(surface, radius) == SC.ref("corner_0.05", 40).m).all()       # the context goes on


def test_estimation_classes(api, ctx):
    """api.NormalEstimation / api.FPFHEstimationOMP with setSearchSurface, from host and device clouds: the bytes of the DeviceCloud
    calls.  setKSearch with a surface is refused as not built; FPFHEstimation has no search surface."""
    from rsreg_amd import lib
    name, pick = "corner_0.05", 40
    q, s, nrm, radius = SC.case(name, pick)
    surface, normals = _surface(api, ctx, name)
    dq = _queries(api, ctx, q)
    want = dq.fpfh_radius_surface_cloud(surface, normals, radius).download_fpfh().points.tobytes()
    want_n = dq.normals_radius_surface_cloud(surface, radius, (0.1, 0.2, 3.0)).download_normals().points.tobytes()
    host_q, host_s = _cloud(np.asarray(q), width=19, height=3, seed=1), _cloud(np.asarray(s), seed=2)
    ne = api.NormalEstimation()
    ne.setRadiusSearch(radius)
    ne.setViewPoint(0.1, 0.2, 3.0)
    fe = api.FPFHEstimationOMP()
    fe.setRadiusSearch(radius)
    fe.setInputNormals(_normal_cloud(api, nrm))
    for cin, csurf in ((dq, surface), (host_q, host_s), (dq, host_s), (host_q, surface)):
        ne.setInputCloud(cin)
        ne.setSearchSurface(csurf)
        fe.setInputCloud(cin)
        fe.setSearchSurface(csurf)
        got_n, got = ne.compute(), fe.compute()
        if cin is dq:
            got_n, got = got_n.download_normals(), got.download_fpfh()
        else:
            assert (got.width, got.height, got.is_dense) == (19, 3, False) and (got_n.width, got_n.height) == (19, 3)
        assert got_n.points.tobytes() == want_n and got.points.tobytes() == want
    fe.setInputNormals(normals)                                                   # the surface's normals in HBM
    fe.setInputCloud(dq)
    fe.setSearchSurface(surface)
    assert fe.compute().download_fpfh().points.tobytes() == want
    for est in (ne, fe):
        est.setRadiusSearch(0)
        est.setKSearch(10)
        with pytest.raises(lib.RsregError, match="not built") as e:
            est.compute()
        assert e.value.status == lib.RSREG_ERR_INVALID_ARG
        est.setSearchSurface(None)                                                # without a surface nothing has changed
    ne.setInputCloud(surface)
    assert ne.compute().download_normals().points.tobytes() == surface.normals_cloud(10, (0.1, 0.2, 3.0)).download_normals().points.tobytes()
    with pytest.raises(lib.RsregError, match="not built"):
        api.FPFHEstimation().setSearchSurface(surface)


def test_cpp_adaptor(api, ctx, tmp_path):
    """tests/cpp/surface_runner.cpp (rsreg::NormalEstimation and rsreg::FPFHEstimationOMP with setSearchSurface) gives the bytes of
    the Python path, from host clouds and from device clouds; setKSearch with a surface is refused."""
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "surface_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "surface_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    r = subprocess.run([exe, "refuse"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "refused yes", r.stdout
    xyz, _ = K.holes()
    q = np.asarray(SC.queries("holes", 20))
    surface_cloud, query_cloud = _cloud(xyz, width=50, height=30, is_dense=True), _cloud(q, seed=2)
    surface, dq = api.DeviceCloud(surface_cloud, ctx=ctx), api.DeviceCloud(query_cloud, ctx=ctx)
    nd = surface.normals_radius_cloud(0.15)
    want = dq.fpfh_radius_surface_cloud(surface, nd, 0.2).download_fpfh()
    want_n = dq.normals_radius_surface_cloud(surface, 0.15).download_normals()
    surface_cloud.points.tofile(str(tmp_path / "surface.bin"))
    query_cloud.points.tofile(str(tmp_path / "queries.bin"))
    r = subprocess.run([exe, str(tmp_path / "queries.bin"), str(len(q)), str(tmp_path / "surface.bin"), "50", "30", "0.15", "0.2", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    vals = dict(l.split() for l in r.stdout.strip().splitlines())
    for name in ("fpfh_host.bin", "fpfh_dev.bin"):
        assert open(str(tmp_path / name), "rb").read() == want.points.tobytes()
    assert open(str(tmp_path / "normals_dev.bin"), "rb").read() == want_n.points.tobytes()
    # (the host path's normals: the same radius for the surface's own normals and the queries')
    assert open(str(tmp_path / "normals_host.bin"), "rb").read() == want_n.points.tobytes()
    assert int(vals["size"]) == int(vals["size_device"]) == int(vals["size_normals"]) == len(q)
    assert (int(vals["width"]), int(vals["height"])) == (len(q), 1) and vals["dense"] == vals["dense_device"] == vals["dense_normals"] == "0"
    assert np.isnan(want.points["histogram"]).any(axis=1).sum() >= 2 and np.isfinite(want.points["histogram"]).all(axis=1).sum() >= 50
