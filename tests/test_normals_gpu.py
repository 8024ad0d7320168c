"""rsreg_cloud_knn and rsreg_cloud_normals (pcl::NormalEstimation with setKSearch) on the GPU, the Python and C++ adaptors,
against tests/normals_ref.py.

The search: indices and squared distances BIT-EQUAL to the reference, ties included -- ascending by (d2, original index), the
lowest indices among the records at the k-th distance.

The normals, every finite record of every input (h = 2^-22; C_ref, l0_ref .. l2_ref, n_ref, curv_ref from the reference alone):
  * | |n| - 1 | <= h: a unit vector in double, each component rounded to float (2^-24 relative each);
  * n^T C_ref n - l0_ref <= h * l0_ref + 1e-12 * trace: the Rayleigh quotient, whatever the eigen-gap.  An angle error e adds
    at most e^2 * l2 (float rounding: 3e-15 * trace), the norm (1 +- 2^-23) scales l0, and the two covariances differ by the
    order of their double sums, about 1e-15 of the second moments;
  * |curv - curv_ref| <= 2^-23 * curv_ref + 1e-12: both are floats rounded from doubles that differ by about 1e-15;
  * where gap_ratio = (l1 - l0) / l2 >= 1e-3 (on the reference alone): the angle to +-n_ref is at most 2^-22 rad.  Rounding a
    unit vector to float moves it by at most sqrt(3) * 2^-25 = 5.2e-8; a backward-stable double solve adds about
    1e2 * 2^-53 / 1e-3; the bound is four times the first term -- derived, not measured;
  * the share of records left out by that condition is at most 5 % per input, asserted on the reference.  The lattices are
    exempt from the share (not from the checks): 7 or 27 neighbours of an inner lattice point are a cube, whose covariance is
    a multiple of the identity -- no direction is defined there, by construction (57.9 % of the 12^3 lattice); so is the raw
    frame, whose 6 558 missing-depth records at the origin have all their neighbours in one place (13.1 %; the same frame after
    PassThrough leaves out 0.0 % and is asserted);
  * sign: where the reference has |cos_view| > 1e-6 * |v| (and a gap), n . n_ref > 0; everywhere, n does not point away from
    the viewpoint by more than float rounding.
The search on thin, far, piled-up and cell-aligned clouds (the other rules of the grid's layout): tests/test_pointgrid_searches_gpu.py.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import normals_ref as N
import sor_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 2.0 ** -6
EPS = 2.0 ** -22
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


def _cloud(xyz, width=None, height=1, is_dense=False, seed=0):
    """Records with a colour and a w of their own each: nothing but x, y, z may enter a result."""
    from rsreg_amd import POINT_DTYPE, PointCloud
    rng = np.random.default_rng(seed)
    pts = np.zeros(len(xyz), POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["w"] = rng.random(len(xyz)).astype(np.float32)
    pts["rgba"] = rng.integers(0, 2 ** 32, len(xyz), dtype=np.uint32)
    return PointCloud(pts, width=len(xyz) if width is None else width, height=height, is_dense=is_dense)


def lattice(m):
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)
    return (g * H + np.array([0.0, 0.0, 1.0])).astype(np.float32)


def _uniform(n, seed):
    rng = np.random.default_rng(seed)                       # (the generator of test_sor_gpu.py::test_knn_random_clouds)
    return (rng.random((n, 3)) * np.array([2.0, 1.5, 0.7]) + np.array([-1.0, -0.5, 0.4])).astype(np.float32)


def _sphere(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = 0.5 + 0.002 * rng.standard_normal(n)
    return (np.array([0.1, -0.2, 1.5]) + r[:, None] * u).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _input(name):
    """(PointCloud, asserts the share left out by the gap condition)"""
    from rsreg_amd import PointCloud, synth
    if name == "lattice":
        return _cloud(lattice(12)), False
    if name == "lattice_copies":                            # 70 copies of one point behind the lattice: more zero distances than k
        xyz = lattice(12)
        return _cloud(np.concatenate([xyz, np.repeat(xyz[777][None], 70, axis=0)])), False
    if name == "lattice_pile":                              # 300 copies: the pile alone overfills the 256-element buffer, so the
        xyz = lattice(12)                                   # selection refills in the middle of a cell's run (and the value
        return _cloud(np.concatenate([xyz, np.repeat(xyz[777][None], 300, axis=0)])), False   # search ends right after it)
    if name == "uniform1000":
        return _cloud(_uniform(1000, 1)), True
    if name == "uniform5000":
        return _cloud(_uniform(5000, 2)), True
    if name == "sphere5000":
        return _cloud(_sphere(5000, 3)), True
    if name == "non_finite":
        rng = np.random.default_rng(4)
        xyz = _uniform(3000, 5)
        xyz[rng.integers(0, 3000, 150)] = np.nan
        xyz[rng.integers(0, 3000, 150), 1] = np.inf
        return _cloud(xyz, width=60, height=50), True
    fr = synth.render_frame(1, "50k")                        # raw: the missing-depth records, thousands of them, at the origin
    if name == "frame_raw":
        return fr, False                                    # (the share was measured after PassThrough only: checked there)
    assert name == "frame_pass"
    pts = fr.points[S.passthrough_keep(fr.xyz, 2, 0.2, 2.5)]
    return PointCloud(np.ascontiguousarray(pts), width=len(pts), height=1, is_dense=True), True


@functools.lru_cache(maxsize=None)
def _ref_knn(name, k):
    return N.knn(_input(name)[0].xyz, k)


@functools.lru_cache(maxsize=None)
def _ref_normals(name, k, viewpoint=(0.0, 0.0, 0.0)):
    return N.normals(_input(name)[0].xyz, k, viewpoint, knn_result=_ref_knn(name, k))


SEARCH = ([("lattice", 7), ("lattice", 27), ("lattice_copies", 64), ("lattice_pile", 1), ("lattice_pile", 50), ("lattice_pile", 64)] +
          [(n, k) for n in ("uniform1000", "uniform5000", "sphere5000") for k in (1, 3, 10, 50, 64)] +
          [("non_finite", 20), ("frame_raw", 10), ("frame_raw", 50), ("frame_pass", 10), ("frame_pass", 50)])
NORMALS = [(n, k) for n, k in SEARCH if k >= 3]


# ------------------------------------------------------------------------------------------------ the search
@pytest.mark.parametrize("name,k", SEARCH)
def test_knn_bit_equal(api, ctx, name, k):
    cloud, _ = _input(name)
    idx, d2 = api.DeviceCloud(cloud, ctx=ctx).knn(k)
    want_idx, want_d2 = _ref_knn(name, k)
    bad = np.flatnonzero((idx != want_idx).any(axis=1) | (d2.view(np.uint32) != want_d2.view(np.uint32)).any(axis=1))
    print("knn: %s, n = %d, k = %d, rows that differ: %d" % (name, len(cloud), k, len(bad)))
    assert len(bad) == 0, (bad[:4], idx[bad[:4]], want_idx[bad[:4]], d2[bad[:4]], want_d2[bad[:4]])
    fin = S.finite_rows(cloud.xyz)
    assert (idx[~fin] == -1).all() and (d2[~fin] == 0).all()


def test_knn_lattice_ties_by_hand(api, ctx):
    """An inner lattice point, k = 4: itself, then three of its six neighbours at H -- the three lowest indices.  The copies:
    k = 64 of 71 records in one place are the lowest 64 indices for every one of them."""
    cloud, _ = _input("lattice_copies")
    dc = api.DeviceCloud(cloud, ctx=ctx)
    idx, d2 = dc.knn(4)
    c = (5 * 12 + 5) * 12 + 5
    assert idx[c].tolist() == [c, c - 144, c - 12, c - 1] and d2[c].tolist() == [0.0, H * H, H * H, H * H]
    idx, d2 = dc.knn(64)
    pile = [777] + list(range(1728, 1728 + 70))
    assert (idx[pile] == np.array(pile[:64], np.int32)).all() and (d2[pile] == 0).all()
    only_idx = np.zeros((len(cloud), 64), np.int32)          # each output is nullable
    from rsreg_amd import lib
    lib.check(lib.lib().rsreg_cloud_knn(ctx.h, dc.h, 64, only_idx.ctypes.data, None), ctx.h)
    assert (only_idx == idx).all()


@pytest.mark.parametrize("name,k", [("uniform5000", 50), ("non_finite", 20), ("frame_raw", 50), ("lattice_copies", 64),
                                     ("lattice_pile", 64), ("lattice_pile", 2)])
def test_search_within_sor(api, ctx, name, k):
    """sqrt and mean of d2[:, 1:] are knn_mean_distance(k - 1), bit for bit: the new search and the old one see the same values."""
    dc = api.DeviceCloud(_input(name)[0], ctx=ctx)
    _, d2 = dc.knn(k)
    root = np.sqrt(d2[:, 1:]).astype(np.float64)
    want = (np.cumsum(root, axis=1)[:, -1] / float(k - 1)).astype(np.float32)
    got = dc.knn_mean_distance(k - 1)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


# ------------------------------------------------------------------------------------------------ the normals
def _check_normals(got, cloud, ref, viewpoint, assert_share, label):
    xyz = cloud.xyz
    fin = ref.finite
    assert (fin == S.finite_rows(xyz)).all()
    assert np.isnan(got[~fin]).all()
    n = got[fin, :3].astype(np.float64)
    curv = got[fin, 3]
    C, w, tr = ref.C[fin], ref.evals[fin], ref.trace[fin]
    assert np.isfinite(got[fin]).all()
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
    print("%s: finite %d, |n|-1 %.3g, Rayleigh slack %.3g, curvature slack %.3g, max angle %.3g rad over %d, left out %.2f %%, clear sign %d" %
          (label, int(fin.sum()), norm_err, rq_slack, curv_slack, angle[gap_ok].max() if gap_ok.any() else 0.0, int(gap_ok.sum()),
           100 * out_share, int(clear.sum())))
    assert norm_err <= EPS
    assert rq_slack <= 0
    assert curv_slack <= 0
    assert (angle[gap_ok] <= EPS).all()
    if assert_share:
        assert out_share <= 0.05
    assert ((nn[clear] * nref[clear]).sum(axis=1) > 0).all()
    assert (towards >= -1e-6 * vlen).all()
    flat = tr == 0                                            # all k neighbours in one place: (0, 0, 1) before the flip
    if flat.any():
        want = np.where((ref.cos[fin][flat] < 0)[:, None], np.float32([0, 0, -1]), np.float32([0, 0, 1]))
        assert (got[fin][flat, :3] == want).all() and (curv[flat] == 0).all()


@pytest.mark.parametrize("name,k", NORMALS)
def test_normals_against_the_reference(api, ctx, name, k):
    cloud, share = _input(name)
    got = api.DeviceCloud(cloud, ctx=ctx).normals(k)
    assert got.shape == (len(cloud), 4) and got.dtype == np.float32
    _check_normals(got, cloud, _ref_normals(name, k), (0.0, 0.0, 0.0), share, "%s k=%d" % (name, k))


def test_viewpoint_flips_the_expected_subset(api, ctx):
    vp = (0.3, -0.2, 5.0)
    for name in ("sphere5000", "frame_pass"):
        cloud, share = _input(name)
        dc = api.DeviceCloud(cloud, ctx=ctx)
        a, b = dc.normals(10), dc.normals(10, viewpoint=vp)
        ref_a, ref_b = _ref_normals(name, 10), _ref_normals(name, 10, vp)
        _check_normals(b, cloud, ref_b, vp, share, "%s k=10 viewpoint" % name)
        flipped = (a[:, :3] == -b[:, :3]).all(axis=1) & (a[:, :3] != b[:, :3]).any(axis=1)
        same = (a[:, :3] == b[:, :3]).all(axis=1)
        assert (flipped | same).all() and (a[:, 3] == b[:, 3]).all()
        want = ((ref_a.cos < 0) != (ref_b.cos < 0))
        clear = (ref_a.gap >= 1e-3) & (np.abs(ref_a.cos) > 1e-5) & (np.abs(ref_b.cos) > 1e-5)
        assert (flipped[clear] == want[clear]).all() and flipped.any() and (name != "sphere5000" or not flipped.all())


def test_output_cloud(api, ctx):
    from rsreg_amd import lib
    for name, dense_in in (("non_finite", True), ("uniform1000", True), ("uniform1000", False), ("frame_raw", False)):
        cloud, _ = _input(name)
        cloud = type(cloud)(cloud.points, cloud.width, cloud.height, dense_in)
        dc = api.DeviceCloud(cloud, ctx=ctx)
        ne = api.NormalEstimation()
        ne.setInputCloud(dc)
        ne.setKSearch(10)
        out = ne.compute()
        n, stride, w, h, dense = out.info()
        assert (n, stride, w, h) == (len(cloud), 32, cloud.width, cloud.height)
        rec = out.download_normals().points
        raw = rec.view(np.uint32).reshape(len(cloud), 8)
        assert (raw[:, 3] == 0).all() and (raw[:, 5:] == 0).all()
        nan_rows = np.isnan(rec["normal_x"])
        assert (nan_rows == ~S.finite_rows(cloud.xyz)).all()
        assert (raw[nan_rows][:, [0, 1, 2, 4]] == 0x7fc00000).all()                  # the quiet NaN, four times
        assert dense == (False if nan_rows.any() else dense_in)
        again = ne.compute().download_normals().points
        assert rec.tobytes() == again.tobytes()
        # a context that has indexed a different cloud first
        other = api.Context(0)
        api.DeviceCloud(_input("sphere5000")[0], ctx=other).normals(50)
        fresh = api.DeviceCloud(cloud, ctx=other).normals_cloud(10).download_normals().points
        assert rec.tobytes() == fresh.tobytes()
        four = dc.normals(10)
        assert four.tobytes() == np.stack([rec["normal_x"], rec["normal_y"], rec["normal_z"], rec["curvature"]], 1).tobytes()
    assert lib.lib().rsreg_version() == 4


def test_errors_leave_out_unchanged(api, ctx):
    from rsreg_amd import lib
    L = lib.lib()
    xyz = _uniform(40, 8)
    dc = api.DeviceCloud(_cloud(xyz), ctx=ctx)
    out = api.DeviceCloud(_cloud(_uniform(7, 9)), ctx=ctx)
    before, stamp = out.download().points.tobytes(), out.stamp
    inv = lib.RSREG_ERR_INVALID_ARG
    idx, d2 = np.zeros((40, 64), np.int32), np.zeros((40, 64), np.float32)
    assert L.rsreg_cloud_normals(ctx.h, dc.h, 2, None, out.h) == inv
    assert L.rsreg_cloud_normals(ctx.h, dc.h, 65, None, out.h) == inv
    assert L.rsreg_cloud_normals(ctx.h, dc.h, 41, None, out.h) == inv                # more than the cloud holds
    assert L.rsreg_cloud_normals(ctx.h, dc.h, 10, None, dc.h) == inv                 # out == in
    assert L.rsreg_cloud_normals(ctx.h, dc.h, 10, None, None) == inv
    assert L.rsreg_cloud_knn(ctx.h, dc.h, 0, idx.ctypes.data, d2.ctypes.data) == inv
    assert L.rsreg_cloud_knn(ctx.h, dc.h, 65, idx.ctypes.data, d2.ctypes.data) == inv
    assert L.rsreg_cloud_knn(ctx.h, dc.h, 41, idx.ctypes.data, d2.ctypes.data) == inv
    xyz[:5] = np.nan
    holes = api.DeviceCloud(_cloud(xyz), ctx=ctx)
    assert L.rsreg_cloud_normals(ctx.h, holes.h, 36, None, out.h) == inv             # 35 finite records
    assert L.rsreg_cloud_knn(ctx.h, holes.h, 36, idx.ctypes.data, d2.ctypes.data) == inv
    other = api.Context(0)
    foreign_in, foreign_out = api.DeviceCloud(_cloud(xyz), ctx=other), api.DeviceCloud(ctx=other)
    assert L.rsreg_cloud_normals(ctx.h, foreign_in.h, 10, None, out.h) == inv       # a cloud of another context
    assert L.rsreg_cloud_normals(ctx.h, dc.h, 10, None, foreign_out.h) == inv
    assert L.rsreg_cloud_knn(ctx.h, foreign_in.h, 10, idx.ctypes.data, d2.ctypes.data) == inv
    assert out.download().points.tobytes() == before and out.stamp == stamp and len(dc) == 40
    with pytest.raises(lib.RsregError) as e:
        dc.normals(2)
    assert e.value.status == inv
    lib.check(L.rsreg_cloud_normals(ctx.h, holes.h, 35, None, out.h), ctx.h)         # exactly k finite records
    assert out.stamp[1] != stamp[1] and out.info()[:2] == (40, 32)
    i35, _ = holes.knn(35)
    assert (np.sort(i35[5:], axis=1) == np.arange(5, 40)).all()


def test_adaptors(api, ctx, tmp_path):
    """tests/cpp/normals_runner.cpp gives the bytes of the Python path, from host clouds and from device clouds; so does
    api.NormalEstimation on a host cloud."""
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "normals_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "normals_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    fr, _ = _input("frame_raw")
    vp = (0.3, -0.2, 5.0)
    want = api.DeviceCloud(fr, ctx=ctx).normals_cloud(20, vp).download_normals()
    ne = api.NormalEstimation()
    ne.setInputCloud(fr)                                     # a host cloud: through a temporary DeviceCloud
    ne.setKSearch(20)
    ne.setViewPoint(*vp)
    host = ne.compute()
    assert host.points.tobytes() == want.points.tobytes()
    assert (host.width, host.height, host.is_dense) == (fr.width, fr.height, False) == (want.width, want.height, want.is_dense)
    fr.points.tofile(str(tmp_path / "in.bin"))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(fr.width), str(fr.height), "20", "0.3", "-0.2", "5", str(tmp_path / "host.bin"),
                        str(tmp_path / "dev.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    vals = dict(l.split() for l in r.stdout.strip().splitlines())
    for name in ("host.bin", "dev.bin"):
        assert open(str(tmp_path / name), "rb").read() == want.points.tobytes()
    assert int(vals["size"]) == int(vals["size_device"]) == len(fr) and int(vals["width"]) == fr.width and int(vals["height"]) == fr.height
    assert vals["dense"] == vals["dense_device"] == "0" and vals["k"] == "20"
