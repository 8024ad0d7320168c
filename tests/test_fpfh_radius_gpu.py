"""rsreg_cloud_spfh_radius and rsreg_cloud_fpfh_radius (pcl::FPFHEstimationOMP with setRadiusSearch) on the GPU, the Python and C++
adaptors, against tests/fpfh_radius_ref.py on the cases of tests/fpfh_radius_cases.py.

The same float32 normals go to the engine and to the reference.  On every record that is not fragile the SPFH rows and the neighbour
counts are BIT-EQUAL.  On every record that is not fragile and has no fragile neighbour the FPFH values are within ONE float32 step
of the reference, with the same NaN mask.  The step is derived, not measured: either side adds at most m non-negative doubles, a
relative error of at most about (2 m + 4) * 2^-53 each -- below 2^-32 for m up to 10^6, against a half-step of 2^-25 -- so either
side rounds to the correct float or to its neighbour.  And at most 1 value in 10 000 may differ at all: a contracted multiply-add or
a float accumulator cannot hide inside the step.  The conditions on the inputs (how many records may be fragile, how many values the
order of the sums may move) are checked on the reference alone in tests/test_fpfh_radius_cpu.py and again here.
"""
import os
import subprocess

import numpy as np
import pytest

import fpfh_cases as K
import fpfh_radius_cases as C
import fpfh_radius_ref as FR
import fpfh_ref as F
import radius_ref as R

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


def _cloud(xyz, width=None, height=1, is_dense=True, seed=0):
    """Records with a colour and a w of their own each: nothing but x, y, z may enter a result."""
    from rsreg_amd import POINT_DTYPE, PointCloud
    rng = np.random.default_rng(seed)
    pts = np.zeros(len(xyz), POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["w"] = rng.random(len(xyz)).astype(np.float32)
    pts["rgba"] = rng.integers(0, 2 ** 32, len(xyz), dtype=np.uint32)
    return PointCloud(pts, width=len(xyz) if width is None else width, height=height, is_dense=is_dense)


def _records(api, first3, floats, width=None, height=1, fill=7.0):
    """(n, 3) float32 -> a host cloud of records of `floats` floats each that begin with them (the rest: `fill`)"""
    rec = np.full((len(first3), floats), fill, np.float32)
    rec[:, :3] = first3
    raw = np.ascontiguousarray(rec).view(np.dtype((np.void, floats * 4))).reshape(-1)
    return api.NormalCloud(raw, len(raw) if width is None else width, height, True)


def _normal_cloud(api, nrm):
    rec = np.zeros(len(nrm), api.NORMAL_DTYPE)
    rec["normal_x"], rec["normal_y"], rec["normal_z"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    rec["curvature"] = 0.25
    return api.NormalCloud(rec, len(rec), 1, True)


def _xyz3(rec):
    return np.stack([rec["normal_x"], rec["normal_y"], rec["normal_z"]], axis=1)


def _differing(a, b):
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())


def _check(got, spfh, m, ref, label, rows=None):
    """The rule of the module's docstring on `rows` (all of them if None); prints each figure before it asserts."""
    rows = np.arange(len(ref.m)) if rows is None else np.asarray(rows)
    g, s, mm = got[rows], spfh[rows], m[rows]
    want, want_s, want_m = ref.fpfh[rows], ref.spfh[rows], ref.m[rows]
    sound, ok = ~ref.fragile[rows], ~ref.fragile_nb[rows]
    differ = _differing(np.ascontiguousarray(g[ok]), np.ascontiguousarray(want[ok]))
    both = ok[:, None] & ~np.isnan(g) & ~np.isnan(want)
    steps = FR.ulp_apart(np.ascontiguousarray(g[both]), np.ascontiguousarray(want[both]))
    print("%s: rows %d, fragile %d, fragile or beside one %d, SPFH rows that differ %d, counts that differ %d, FPFH values that differ %d "
          "of %d, largest distance %d steps" % (label, len(rows), int((~sound).sum()), int((~ok).sum()), int((s[sound] != want_s[sound]).any(axis=1).sum()),
                                                int((mm != want_m).sum()), differ, int(ok.sum()) * 33, int(steps.max()) if len(steps) else 0))
    assert (~sound).mean() <= C.FRAGILE_CAP and (~ok).mean() <= C.FRAGILE_NB_CAP
    assert (mm == want_m).all()
    assert s[sound].tobytes() == want_s[sound].tobytes()
    assert (np.isnan(g[ok]) == np.isnan(want[ok])).all()
    assert (steps <= 1).all()
    assert differ <= C.DIFFER_CAP * int(ok.sum()) * 33
    nan_rows = ref.nan_rows[rows]
    assert (g[nan_rows].view(np.uint32) == QNAN).all() and (s[nan_rows] == 0).all()
    rest = ~ok & ~np.isnan(g).any(axis=1)
    assert F.blocks_ok(g[rest]).all()
    assert F.blocks_ok(g[~np.isnan(g).any(axis=1)]).all()


_DEV = {}


def _device(api, ctx, name):
    """(DeviceCloud, NormalCloud) of a case, uploaded once"""
    if name not in _DEV:
        xyz, nrm, _ = C.case(name)
        _DEV[name] = (api.DeviceCloud(_cloud(xyz), ctx=ctx), _normal_cloud(api, nrm))
    return _DEV[name]


EQUAL = ["corner_0.05", "corner_0.12", "corner_0.25", "sphere_0.2", "uniform_0.12", "copies_0.12", "pile", "holes", "at_the_radius", "denormal"]


@pytest.mark.parametrize("name", EQUAL)
def test_equal_to_the_reference(api, ctx, name):
    xyz, nrm, radius = C.case(name)
    ref = C.ref(name)
    dc, normals = _device(api, ctx, name)
    spfh, m = dc.spfh_radius(normals, radius, counts=True)
    out = dc.fpfh_radius_cloud(normals, radius)
    got = out.download_fpfh().points["histogram"]
    assert got.shape == spfh.shape == (len(xyz), 33) and got.dtype == spfh.dtype == np.float32 and m.dtype == np.uint32
    _check(got, spfh, m, ref, name)
    assert (m == dc.radius_count(radius)).all()
    assert out.info() == (len(xyz), 132, len(xyz), 1, not np.isnan(ref.fpfh).any())
    assert dc.spfh_radius(normals, radius).tobytes() == spfh.tobytes()             # count_out may be NULL
    assert dc.fpfh_radius(normals, radius).tobytes() == got.tobytes()


def test_one_and_two_neighbours(api, ctx):
    """m = 1: no pair, no division by m - 1 = 0, zeros in both rows; m = 2: hist_incr = 100, one 100 per block."""
    xyz, nrm, radius = C.case("uniform_0.12")
    ref = C.ref("uniform_0.12")
    dc, normals = _device(api, ctx, "uniform_0.12")
    spfh, m = dc.spfh_radius(normals, radius, counts=True)
    got = dc.fpfh_radius(normals, radius)
    one, two = m == 1, m == 2
    assert one.sum() == (ref.m == 1).sum() >= 10 and two.sum() == (ref.m == 2).sum() >= 10
    assert (spfh[one].view(np.uint32) == 0).all() and (got[one].view(np.uint32) == 0).all()
    assert np.isin(spfh[two], [0.0, 100.0]).all() and (spfh[two].sum(axis=1) == 300.0).all()


def test_copies_are_counted_and_skipped(api, ctx):
    """Exact copies count in m and are skipped in both passes; a record with twelve copies and nothing else in range gets 33
    zeros twice, and the cloud stays dense."""
    ref = C.ref("copies_0.12")
    dc, normals = _device(api, ctx, "copies_0.12")
    radius = C.case("copies_0.12")[2]
    spfh, m = dc.spfh_radius(normals, radius, counts=True)
    got = dc.fpfh_radius(normals, radius)
    stack = [7] + list(range(1500, 1512))
    assert (m[stack] == ref.m[7]).all() and ref.m[7] > 13
    assert len({got[i].tobytes() for i in stack}) == 1 and len({spfh[i].tobytes() for i in stack}) == 1 and (got[7] != 0).any()
    dc, normals = _device(api, ctx, "pile")
    spfh, m = dc.spfh_radius(normals, 0.12, counts=True)
    out = dc.fpfh_radius_cloud(normals, 0.12)
    got = out.download_fpfh().points["histogram"]
    assert (m[-13:] == 13).all() and (spfh[-13:].view(np.uint32) == 0).all() and (got[-13:].view(np.uint32) == 0).all()
    assert out.info()[4] is True


def test_non_finite_records_and_normals(api, ctx):
    """Zero SPFH rows that still sit in their neighbours' sums, quiet NaN FPFH rows, is_dense 0, width and height kept."""
    xyz, nrm, radius = C.case("holes")
    ref = C.ref("holes")
    dc = api.DeviceCloud(_cloud(xyz, width=50, height=30), ctx=ctx)
    normals = _normal_cloud(api, nrm)
    out = dc.fpfh_radius_cloud(normals, radius)
    assert out.info() == (len(xyz), 132, 50, 30, False)
    got = out.download_fpfh().points["histogram"]
    spfh, m = dc.spfh_radius(normals, radius, counts=True)
    _check(got, spfh, m, ref, "holes, organized")
    assert ref.nan_rows.sum() == 70 and (got[ref.nan_rows].view(np.uint32) == QNAN).all() and not np.isnan(got[~ref.nan_rows]).any()
    assert (m[~np.isfinite(xyz).all(axis=1)] == 0).all()
    # is_dense is the input's where nothing is NaN
    x2, n2, r2 = C.case("uniform_0.12")
    loose = api.DeviceCloud(_cloud(x2, width=30, height=50, is_dense=False), ctx=ctx)
    assert loose.fpfh_radius_cloud(_normal_cloud(api, n2), r2).info() == (len(x2), 132, 30, 50, False)


def test_normals_from_the_engine(api, ctx):
    """Normals of normals_radius at a radius that leaves some records fewer than three neighbours: NaN normals the engine made
    itself.  The reference gets the bytes the engine used."""
    xyz = K.cloud("uniform")
    dc = api.DeviceCloud(_cloud(xyz), ctx=ctx)
    nd = dc.normals_radius_cloud(C.ENGINE_NORMALS_RADIUS)
    nrm = _xyz3(nd.download_normals().points)
    few = R.counts(xyz, C.ENGINE_NORMALS_RADIUS) < 3
    assert 20 <= few.sum() and (np.isnan(nrm).any(axis=1) == few).all()
    ref = FR.fpfh_radius(xyz, nrm, 0.2)
    out = dc.fpfh_radius_cloud(nd, 0.2)
    got = out.download_fpfh().points["histogram"]
    spfh, m = dc.spfh_radius(nd, 0.2, counts=True)
    _check(got, spfh, m, ref, "engine normals")
    assert (np.isnan(got).any(axis=1) == few).all() and out.info()[4] is False


def test_at_the_radius_and_denormal(api, ctx):
    """A record AT the radius on the 2^-6 lattice is no neighbour; a pair at a denormal d2 gets w = +inf and the NaNs the formula
    makes, which clear is_dense."""
    xyz, nrm, radius = C.case("at_the_radius")
    dc, normals = _device(api, ctx, "at_the_radius")
    _, m = dc.spfh_radius(normals, radius, counts=True)
    inner = (6 * 12 + 6) * 12 + 6
    assert m[inner] == 27 and m.max() == 27
    _, m = dc.spfh_radius(normals, float(np.nextafter(np.float32(radius), np.float32(1.0))), counts=True)
    assert m[inner] == 33
    ref = C.ref("denormal")
    dc, normals = _device(api, ctx, "denormal")
    out = dc.fpfh_radius_cloud(normals, 0.12)
    got = out.download_fpfh().points["histogram"]
    assert (np.isnan(got) == np.isnan(ref.fpfh)).all() and np.isnan(got[-2:]).all() and not np.isnan(got[:-2]).any()
    assert out.info()[4] is False


def test_grid_stride_loop(api, ctx):
    """66 000 records, about three neighbours each: more than the 65 536 workgroups of either launch, record ids past 65 535.
    2 000 sampled rows against the reference, every count, and every block of every row."""
    xyz, nrm, radius = C.case("many")
    ref = C.ref("many")
    dc, normals = _device(api, ctx, "many")
    spfh, m = dc.spfh_radius(normals, radius, counts=True)
    got = dc.fpfh_radius(normals, radius)
    rng = np.random.default_rng(21)
    rows = np.concatenate([rng.choice(len(xyz), 1994, replace=False), [0, 1, 65535, 65536, 65999, 65998]])
    _check(got, spfh, m, ref, "many", rows=rows)
    assert (m == ref.m).all()
    assert F.blocks_ok(got).all()


def test_record_layouts(api, ctx):
    """12-, 16- and 48-byte point records, 12- and 32-byte normal records: the same bytes."""
    xyz, nrm, radius = C.case("corner_0.05")
    dc, normals = _device(api, ctx, "corner_0.05")
    first = dc.fpfh_radius(normals, radius).tobytes()
    first_spfh = dc.spfh_radius(normals, radius).tobytes()
    for floats in (3, 4, 12):
        other = api.DeviceCloud(_records(api, xyz, floats), ctx=ctx)
        assert other.info()[1] == 4 * floats
        for nfloats in (3, 8):
            nd = api.DeviceCloud(_records(api, nrm, nfloats, fill=np.nan), ctx=ctx)
            assert nd.info()[1] == 4 * nfloats
            assert other.fpfh_radius(nd, radius).tobytes() == first
            assert other.spfh_radius(nd, radius).tobytes() == first_spfh
    assert dc.fpfh_radius(nrm, radius).tobytes() == first                           # an (n, 3) array: uploaded as 12-byte records


@pytest.mark.parametrize("power", [-20, 20])
def test_scaled_by_a_power_of_two(api, ctx, power):
    """Cloud and radius times 2^power: every quantity of the contract scales by an exact power of two (d2, r2, w, the products,
    the sums) or not at all (the pair features), and w * SPFH stays in range, so the SPFH and FPFH bytes are those of scale 1."""
    xyz, nrm, radius = C.case("corner_0.12")
    dc, normals = _device(api, ctx, "corner_0.12")
    scaled = api.DeviceCloud(_cloud(np.ldexp(xyz, power), seed=3), ctx=ctx)
    r = float(np.ldexp(radius, power))
    spfh, m = scaled.spfh_radius(normals, r, counts=True)
    want_spfh, want_m = dc.spfh_radius(normals, radius, counts=True)
    assert (m == want_m).all() and spfh.tobytes() == want_spfh.tobytes()
    assert scaled.fpfh_radius(normals, r).tobytes() == dc.fpfh_radius(normals, radius).tobytes()


def test_determinism(api, ctx):
    xyz, nrm, radius = C.case("corner_0.12")
    dc, normals = _device(api, ctx, "corner_0.12")
    first = dc.fpfh_radius_cloud(normals, radius).download_fpfh().points.tobytes()
    assert dc.fpfh_radius_cloud(normals, radius).download_fpfh().points.tobytes() == first      # a second call
    other = api.Context(0)                                                # a fresh context that first indexed another cloud at another radius
    sx, sn, sr = C.case("sphere_0.2")
    sph = api.DeviceCloud(_cloud(sx), ctx=other)
    sph.fpfh_radius(_normal_cloud(api, sn), sr)
    sph.fpfh(_normal_cloud(api, sn), 50)
    there = api.DeviceCloud(_cloud(xyz, seed=5), ctx=other)
    assert there.fpfh_radius_cloud(_normal_cloud(api, nrm), radius).download_fpfh().points.tobytes() == first


def test_estimation_class(api, ctx):
    """api.FPFHEstimationOMP: the radius path from device and host clouds, the k path with the bytes of rsreg_cloud_fpfh, both
    searches and neither refused."""
    from rsreg_amd import lib
    xyz, nrm, radius = C.case("corner_0.05")
    dc, normals = _device(api, ctx, "corner_0.05")
    first = dc.fpfh_radius_cloud(normals, radius).download_fpfh().points.tobytes()
    fe = api.FPFHEstimationOMP()
    fe.setNumberOfThreads(8)
    fe.setInputCloud(dc)
    fe.setInputNormals(normals)
    fe.setRadiusSearch(radius)
    assert fe.getRadiusSearch() == radius and fe.getKSearch() == 0
    assert fe.compute().download_fpfh().points.tobytes() == first
    fe.setInputCloud(_cloud(xyz, width=40, height=50))
    host = fe.compute()
    assert host.points.tobytes() == first and (host.width, host.height, host.is_dense) == (40, 50, True)
    fe.setKSearch(10)
    with pytest.raises(lib.RsregError, match="both") as e:
        fe.compute()
    assert e.value.status == lib.RSREG_ERR_INVALID_ARG
    fe.setRadiusSearch(0)
    fe.setInputCloud(dc)
    assert fe.compute().download_fpfh().points.tobytes() == dc.fpfh_cloud(normals, 10).download_fpfh().points.tobytes()
    fe.setKSearch(0)
    with pytest.raises(lib.RsregError, match="neither"):
        fe.compute()


def test_refusals(api, ctx):
    from rsreg_amd import lib
    L = lib.lib()
    inv = lib.RSREG_ERR_INVALID_ARG
    xyz = K.uniform(40, 8)
    dc = api.DeviceCloud(_cloud(xyz), ctx=ctx)
    nd = dc.normals_cloud(10)
    out = api.DeviceCloud(_cloud(K.uniform(7, 9)), ctx=ctx)
    before, stamp = out.download().points.tobytes(), out.stamp
    host = np.zeros((40, 33), np.float32)
    cnt = np.zeros(40, np.uint32)
    for radius in (0.0, -0.1, float("nan"), float("inf"), float("-inf")):
        assert L.rsreg_cloud_fpfh_radius(ctx.h, dc.h, nd.h, radius, out.h) == inv
        assert L.rsreg_cloud_spfh_radius(ctx.h, dc.h, nd.h, radius, host.ctypes.data, cnt.ctypes.data) == inv
    assert L.rsreg_cloud_fpfh_radius(ctx.h, dc.h, nd.h, 0.1, dc.h) == inv                   # out == in
    assert L.rsreg_cloud_fpfh_radius(ctx.h, dc.h, nd.h, 0.1, nd.h) == inv                   # out == normals
    assert L.rsreg_cloud_fpfh_radius(ctx.h, dc.h, nd.h, 0.1, None) == inv
    assert L.rsreg_cloud_fpfh_radius(ctx.h, dc.h, None, 0.1, out.h) == inv
    assert L.rsreg_cloud_fpfh_radius(ctx.h, None, nd.h, 0.1, out.h) == inv
    assert L.rsreg_cloud_fpfh_radius(None, dc.h, nd.h, 0.1, out.h) == inv
    assert L.rsreg_cloud_spfh_radius(ctx.h, dc.h, nd.h, 0.1, None, cnt.ctypes.data) == inv
    assert L.rsreg_cloud_spfh_radius(ctx.h, dc.h, None, 0.1, host.ctypes.data, None) == inv
    assert L.rsreg_cloud_spfh_radius(ctx.h, None, nd.h, 0.1, host.ctypes.data, None) == inv
    short = api.DeviceCloud(_normal_cloud(api, C._unit(39, 1)), ctx=ctx)                    # normals of n - 1 records
    assert L.rsreg_cloud_fpfh_radius(ctx.h, dc.h, short.h, 0.1, out.h) == inv
    assert L.rsreg_cloud_spfh_radius(ctx.h, dc.h, short.h, 0.1, host.ctypes.data, cnt.ctypes.data) == inv
    other = api.Context(0)
    foreign = api.DeviceCloud(_normal_cloud(api, C._unit(40, 2)), ctx=other)
    assert L.rsreg_cloud_fpfh_radius(ctx.h, dc.h, foreign.h, 0.1, out.h) == inv             # normals of another context
    assert L.rsreg_cloud_spfh_radius(ctx.h, dc.h, foreign.h, 0.1, host.ctypes.data, None) == inv
    far = api.DeviceCloud(ctx=other)
    assert L.rsreg_cloud_fpfh_radius(ctx.h, dc.h, nd.h, 0.1, far.h) == inv                  # an output of another context
    assert out.download().points.tobytes() == before and out.stamp == stamp and (host == 0).all() and (cnt == 0).all()
    with pytest.raises(lib.RsregError) as e:
        dc.fpfh_radius(nd, 0.0)
    assert e.value.status == inv
    lib.check(L.rsreg_cloud_fpfh_radius(ctx.h, dc.h, nd.h, 0.1, out.h), ctx.h)             # ... and the context goes on
    assert out.stamp == (stamp[0], stamp[1] + 1) and out.info()[:4] == (40, 132, 40, 1)
    assert L.rsreg_version() == 4


def test_empty_and_no_finite_record(api, ctx):
    """As rsreg_cloud_normals_radius: an empty cloud gives an empty cloud of 132-byte records, a cloud without a finite record NaN
    rows, zero SPFH rows and zero counts, nothing launched; the context goes on."""
    empty = api.DeviceCloud(_cloud(np.zeros((0, 3), np.float32)), ctx=ctx)
    none = api.DeviceCloud(_normal_cloud(api, np.zeros((0, 3), np.float32)), ctx=ctx)
    out = empty.fpfh_radius_cloud(none, 0.1)
    assert out.info()[0] == 0 and len(out.download_fpfh().points) == 0
    spfh, m = empty.spfh_radius(none, 0.1, counts=True)
    assert spfh.shape == (0, 33) and len(m) == 0
    xyz = np.full((70, 3), np.nan, np.float32)
    xyz[::3, 1] = np.inf
    dc = api.DeviceCloud(_cloud(xyz, width=10, height=7), ctx=ctx)
    normals = _normal_cloud(api, C._unit(70, 4))
    out = dc.fpfh_radius_cloud(normals, 0.5)
    assert out.info() == (70, 132, 10, 7, False)
    assert (out.download_fpfh().points["histogram"].view(np.uint32) == QNAN).all()
    spfh, m = dc.spfh_radius(normals, 0.5, counts=True)
    assert (spfh.view(np.uint32) == 0).all() and (m == 0).all()
    ref = C.ref("corner_0.05")
    cd, cn = _device(api, ctx, "corner_0.05")
    s2, m2 = cd.spfh_radius(cn, 0.05, counts=True)
    assert (m2 == ref.m).all() and s2[~ref.fragile].tobytes() == ref.spfh[~ref.fragile].tobytes()


def test_cpp_adaptor(api, ctx, tmp_path):
    """tests/cpp/fpfh_radius_runner.cpp (rsreg::NormalEstimation::setRadiusSearch -> rsreg::FPFHEstimationOMP::setRadiusSearch)
    gives the bytes of the Python path, from host clouds and from device clouds; with setKSearch the bytes of rsreg_cloud_fpfh."""
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "fpfh_radius_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fpfh_radius_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    xyz, _ = K.holes()
    cloud = _cloud(xyz, width=50, height=30, is_dense=False)
    dc = api.DeviceCloud(cloud, ctx=ctx)
    nd = dc.normals_radius_cloud(0.15)
    want = dc.fpfh_radius_cloud(nd, 0.2).download_fpfh()
    want_k = dc.fpfh_cloud(nd, 16).download_fpfh()
    cloud.points.tofile(str(tmp_path / "in.bin"))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), "50", "30", "0.15", "0.2", "16", str(tmp_path / "host.bin"), str(tmp_path / "dev.bin"),
                        str(tmp_path / "k.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    vals = dict(l.split() for l in r.stdout.strip().splitlines())
    for name in ("host.bin", "dev.bin"):
        assert open(str(tmp_path / name), "rb").read() == want.points.tobytes()
    assert open(str(tmp_path / "k.bin"), "rb").read() == want_k.points.tobytes()
    assert int(vals["size"]) == int(vals["size_device"]) == int(vals["size_k"]) == len(xyz)
    assert (int(vals["width"]), int(vals["height"])) == (50, 30) and vals["dense"] == vals["dense_device"] == "0"
    assert float(vals["radius"]) == 0.2 and vals["k"] == "16" and not want.is_dense
    assert np.isnan(want.points["histogram"]).any(axis=1).sum() >= 40 and np.isfinite(want.points["histogram"]).all(axis=1).sum() >= 1000
