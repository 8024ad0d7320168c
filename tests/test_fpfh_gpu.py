"""rsreg_cloud_spfh and rsreg_cloud_fpfh (pcl::FPFHEstimation with setKSearch) on the GPU, the Python and C++ adaptors, against
tests/fpfh_ref.py.

The normals come from rsreg_cloud_normals at k = 10 (hand-made ones where a cloud is too small for that); the same bytes go to
the GPU call and to the reference.  SPFH rows are EQUAL on every record that is not fragile, FPFH rows BIT-EQUAL on every record
that is not fragile and has no fragile neighbour (fragile: a pair feature within 1e-9 bins of a bin edge, decided on the reference
alone; tests/fpfh_ref.py derives the figure).  Every other record is finite and its blocks sum to 100 +- 1e-3 or are zero.
The cases of fpfh_cases.HAND_MADE feed normals that are not unit vectors -- scaled, all (0, 0, 1), two of them zero -- through the
same rule: the clamps of the bins, the |v| = 0 skip and atan2(+-0, +-0) are reached by nothing else.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import fpfh_cases as K
import fpfh_ref as F
import normals_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def _cloud(xyz, width=None, height=1, is_dense=True, seed=0):
    """Records with a colour and a w of their own each: nothing but x, y, z may enter a result."""
    from rsreg_amd import POINT_DTYPE, PointCloud
    rng = np.random.default_rng(seed)
    pts = np.zeros(len(xyz), POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["w"] = rng.random(len(xyz)).astype(np.float32)
    pts["rgba"] = rng.integers(0, 2 ** 32, len(xyz), dtype=np.uint32)
    return PointCloud(pts, width=len(xyz) if width is None else width, height=height, is_dense=is_dense)


def _normal_cloud(api, nrm):
    """(n, 3) float32 -> a NormalCloud of 32-byte pcl::Normal records"""
    rec = np.zeros(len(nrm), api.NORMAL_DTYPE)
    rec["normal_x"], rec["normal_y"], rec["normal_z"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    return api.NormalCloud(rec, len(rec), 1, True)


def _xyz3(rec):
    return np.stack([rec["normal_x"], rec["normal_y"], rec["normal_z"]], axis=1)


_STATE = {}


def _case(api, ctx, name):
    """(xyz, DeviceCloud, its normals at k = 10 as a DeviceCloud, the same normals on the host (n, 3)), made once per case."""
    if name not in _STATE:
        xyz = K.many() if name == "many" else K.cloud(name)
        dc = api.DeviceCloud(_cloud(xyz), ctx=ctx)
        nd = dc.normals_cloud(10)
        _STATE[name] = (xyz, dc, nd, _xyz3(nd.download_normals().points))
    return _STATE[name]


@functools.lru_cache(maxsize=None)
def _ref_cached(name, k):
    xyz, _, _, nrm = _STATE[name]
    return F.fpfh(xyz, nrm, k)


def _ref(api, ctx, name, k):
    _case(api, ctx, name)
    return _ref_cached(name, k)


def _check_fpfh(got, ref, label):
    ok = ~ref.fragile_nb & ~ref.nan_rows
    bad = np.flatnonzero((got[ok].view(np.uint32) != ref.fpfh[ok].view(np.uint32)).any(axis=1))
    print("%s: records %d, fragile %d, fragile or fragile neighbour %d, rows that differ %d" %
          (label, len(got), int(ref.fragile.sum()), int(ref.fragile_nb.sum()), len(bad)))
    assert len(bad) == 0, (np.flatnonzero(ok)[bad[:4]], got[ok][bad[:4]], ref.fpfh[ok][bad[:4]])
    rest = ~ok & ~ref.nan_rows
    assert np.isfinite(got[rest]).all() and F.blocks_ok(got[rest]).all()
    assert np.isnan(got[ref.nan_rows]).all()
    assert F.blocks_ok(got[~ref.nan_rows]).all()


SPFH = [("uniform", 2), ("uniform", 10), ("uniform", 33), ("uniform", 64), ("sphere", 16), ("corner", 10), ("plane", 9)]


@pytest.mark.parametrize("name,k", SPFH)
def test_spfh_equal(api, ctx, name, k):
    xyz, dc, nd, _ = _case(api, ctx, name)
    ref = _ref(api, ctx, name, k)
    got = dc.spfh(nd, k)
    assert got.shape == (len(xyz), 33) and got.dtype == np.float32
    ok = ~ref.fragile
    print("spfh %s k=%d: fragile %d of %d" % (name, k, int(ref.fragile.sum()), len(xyz)))
    np.testing.assert_array_equal(got[ok], ref.spfh[ok])
    assert ok.mean() >= 0.99                                   # (two mutual neighbours of the shell may get opposite normals: theta = pi)


@pytest.mark.parametrize("name,k", SPFH + [("lattice", 10)])
def test_fpfh_bit_equal(api, ctx, name, k):
    xyz, dc, nd, _ = _case(api, ctx, name)
    ref = _ref(api, ctx, name, k)
    got = dc.fpfh(nd, k)
    assert got.shape == (len(xyz), 33) and got.dtype == np.float32
    _check_fpfh(got, ref, "fpfh %s k=%d" % (name, k))


def test_plane_lattice_ties(api, ctx):
    """Distance ties everywhere: the bytes equal the reference's, so the neighbour order (d2, index) is the order the float sums
    ran in.  No record of the plane is fragile -- every feature sits at mid-bin."""
    xyz, dc, nd, _ = _case(api, ctx, "plane")
    ref = _ref(api, ctx, "plane", 9)
    assert not ref.fragile_nb.any() and not ref.nan_rows.any()
    inner = 15 * 30 + 15
    assert (ref.d2[inner, 1:5] == ref.d2[inner, 1]).all() and (ref.d2[inner, 5:9] == ref.d2[inner, 5]).all()   # four at H, four at H * sqrt(2)
    assert dc.fpfh(nd, 9).tobytes() == ref.fpfh.tobytes()
    assert dc.spfh(nd, 9).tobytes() == ref.spfh.tobytes()


def _hand_made(api, ctx, name, k=10):
    """(DeviceCloud, NormalCloud, reference) of a case of fpfh_cases.HAND_MADE: the same float32 normals go to both."""
    xyz, nrm = K.HAND_MADE[name]()
    return api.DeviceCloud(_cloud(xyz), ctx=ctx), _normal_cloud(api, nrm), F.fpfh(xyz, nrm, k)


def _check_by_the_rule(dc, normals, ref, k, label):
    """SPFH equal on the records that are not fragile, FPFH by _check_fpfh; returns both."""
    spfh, got = dc.spfh(normals, k), dc.fpfh(normals, k)
    np.testing.assert_array_equal(spfh[~ref.fragile], ref.spfh[~ref.fragile])
    _check_fpfh(got, ref, label)
    return spfh, got


@pytest.mark.parametrize("name", ["non_unit", "non_unit_2^100"])
def test_normals_that_are_not_unit_vectors(api, ctx, name):
    """Normals times 2^e, e in [-20, 20] (and all times 2^100 more): the contract normalises nothing.  f2 and f3 leave [-1, 1], so
    most pairs land in bin 0 or bin 10 through the clamps -- a clamp that is missing or differs moves a count."""
    dc, normals, ref = _hand_made(api, ctx, name)
    assert not ref.fragile_nb.any() and not ref.nan_rows.any()
    s3 = ref.scaled[..., 2]
    below, above = ref.valid & (s3 < 0), ref.valid & (s3 >= 11)
    assert below.sum() > 1000 and above.sum() > 1000
    spfh, got = _check_by_the_rule(dc, normals, ref, 10, name)
    # a pair below 0 is counted in bin 0 of f3, one at 11 or above in bin 10: the counts of those two bins, through the table
    tab = F.count_table(10)
    want0 = np.bincount(np.nonzero(ref.valid & (s3 < 1))[0], minlength=len(spfh))
    want10 = np.bincount(np.nonzero(ref.valid & (s3 >= 10))[0], minlength=len(spfh))
    np.testing.assert_array_equal(spfh[:, 22], tab[want0])
    np.testing.assert_array_equal(spfh[:, 32], tab[want10])
    assert dc.fpfh_cloud(normals, 10).info() == (len(got), 132, len(got), 1, True)   # (finite normals of any length: nothing to flag)


def test_dp_parallel_to_the_source_normal(api, ctx):
    """The 12^3 lattice with every normal (0, 0, 1): the neighbours straight above and below give |v| = 0 and are skipped.  No
    record is fragile, so every byte is the reference's.  Record (6, 6, 6) by hand: of its nine neighbours (six at H, the three of
    lowest index at H * sqrt(2)) the two along z are skipped; the five in its own z-plane have f1 = f2 = f3 at mid-bin (bin 5);
    (-1, 0, -1) and (-1, 0, +1) have f3 = -+0.7071 -> 11 * 0.1464 = 1.61 and 9.39, bins 1 and 9."""
    dc, normals, ref = _hand_made(api, ctx, "parallel")
    n = len(ref.idx)
    own = np.arange(n)[:, None]
    assert (~ref.valid & (ref.idx != own)).sum() > 3000 and not ref.fragile.any() and not ref.fragile_nb.any()
    spfh, got = dc.spfh(normals, 10), dc.fpfh(normals, 10)
    assert spfh.tobytes() == ref.spfh.tobytes()
    assert got.tobytes() == ref.fpfh.tobytes()
    inner = (6 * 12 + 6) * 12 + 6
    assert ref.idx[inner].tolist() == [942, 798, 930, 941, 943, 954, 1086, 786, 797, 799]
    tab = F.count_table(10)
    want = np.zeros(33, np.float32)
    want[5], want[11 + 5] = tab[7], tab[7]
    want[22 + 1], want[22 + 5], want[22 + 9] = tab[1], tab[5], tab[1]
    assert spfh[inner].tolist() == want.tolist() and tab[1] == np.float32(100.0) / np.float32(9.0) and 77.7777 < tab[7] < 77.7778


def _block_fragile(ref, rows):
    """(len(rows), 3) bool: whether a counted pair of the record lies within FRAGILE_BELOW bins of an edge of feature t"""
    s = ref.scaled[rows]
    edges = np.arange(1, F.BINS, dtype=np.float64)
    m = np.abs(s[..., None] - edges).min(axis=-1)
    m[..., 0] = np.minimum(m[..., 0], np.minimum(np.abs(s[..., 0]), np.abs(s[..., 0] - float(F.BINS))))
    return ((m < F.FRAGILE_BELOW) & ref.valid[rows][..., None]).any(axis=1)


def test_zero_normals(api, ctx):
    """Two mutual nearest neighbours with the normal (0, 0, 0), which is finite: their own pair has v = 0 and is skipped both ways,
    every other pair of theirs has theta = atan2(+-0, +-0) -- fragile by the reference's rule, in feature 1 alone.  The rule holds
    on the rest, every row is finite, is_dense stays the input's, and their SPFH rows count exactly the pairs the reference counts."""
    dc, normals, ref = _hand_made(api, ctx, "zero_normals")
    zeroed = list(K.ZEROED)
    assert ref.fragile[zeroed].all() and ref.fragile_nb.mean() <= K.FRAGILE_CAP["zero_normals"] and not ref.nan_rows.any()
    spfh, got = _check_by_the_rule(dc, normals, ref, 10, "zero normals")
    assert np.isfinite(got).all() and F.blocks_ok(got).all() and np.isfinite(spfh).all()
    out = dc.fpfh_cloud(normals, 10)
    assert out.info() == (len(got), 132, len(got), 1, True)
    assert out.download_fpfh().points["histogram"].tobytes() == got.tobytes()
    tab = F.count_table(10)
    sound = ~_block_fragile(ref, zeroed)
    assert sound[:, 1:].all() and not sound[:, 0].any()                      # f2 and f3 are sound, f1 hangs on the sign of a zero
    for row, i in enumerate(zeroed):
        pairs = int(ref.valid[i].sum())
        assert pairs == 8                                                      # nine neighbours, one of them the other zero normal
        for t in range(3):
            block = spfh[i, 11 * t:11 * t + 11]
            assert np.isin(block, tab[:10]).all()
            counts = np.searchsorted(tab[:10], block)                          # (the table is increasing: the count behind each float)
            assert (tab[counts] == block).all()
            if sound[row, t]:
                assert counts.tolist() == ref.counts[i, 11 * t:11 * t + 11].tolist()
            assert counts.sum() == pairs == ref.counts[i, 11 * t:11 * t + 11].sum()


def test_every_k(api, ctx):
    """k = 2 .. 64 on 200 records: hist_incr, the table of counts and the `lane < k` masks at every k.  No record is fragile at any
    k (tests/test_fpfh_cpu.py), so every SPFH and FPFH byte is compared."""
    xyz, nrm = K.every_k()
    dc, normals = api.DeviceCloud(_cloud(xyz), ctx=ctx), _normal_cloud(api, nrm)
    knn = N.knn(xyz, 64)
    for k in K.EVERY_K:
        ref = F.fpfh(xyz, nrm, k, knn_result=(knn[0][:, :k], knn[1][:, :k]))
        assert not ref.fragile_nb.any()
        _check_by_the_rule(dc, normals, ref, k, "every k: k = %d" % k)


def test_exact_copies(api, ctx):
    xyz, dc, nd, _ = _case(api, ctx, "copies")
    ref = _ref(api, ctx, "copies", 10)
    got, spfh = dc.fpfh(nd, 10), dc.spfh(nd, 10)
    _check_fpfh(got, ref, "copies k=10")
    np.testing.assert_array_equal(spfh[~ref.fragile], ref.spfh[~ref.fragile])
    pile = [7] + list(range(1500, 1512))                        # 13 records in one place: all ten neighbours are copies
    assert (ref.d2[pile] == 0).all()
    assert (got[pile] == 0).all() and (spfh[pile] == 0).all()
    mixed = [100, 1512, 1513, 1514]                             # 4 in one place: exactly the zero-distance neighbours are skipped
    assert ((ref.d2[mixed] == 0).sum(axis=1) == 4).all() and not ref.fragile_nb[mixed].any()
    assert (got[mixed] != 0).any(axis=1).all() and got[mixed].tobytes() == ref.fpfh[mixed].tobytes()
    assert got[100].tobytes() == got[1512].tobytes()             # the same neighbours, the same d2: the same row


def test_non_finite_inputs(api, ctx):
    xyz, bad_normals = K.holes()
    dc = api.DeviceCloud(_cloud(xyz, width=50, height=30), ctx=ctx)
    nrm = _xyz3(dc.normals_cloud(10).download_normals().points)
    assert np.isnan(nrm[~N.finite_rows(xyz)]).all()
    nrm[bad_normals[:20]] = np.nan
    nrm[bad_normals[20:], 2] = np.inf
    normals = _normal_cloud(api, nrm)
    ref = F.fpfh(xyz, nrm, 10)
    want_nan = ~N.finite_rows(xyz)
    want_nan[bad_normals] = True
    assert (ref.nan_rows == want_nan).all() and want_nan.sum() == 70
    out = dc.fpfh_cloud(normals, 10)
    n, stride, w, h, dense = out.info()
    assert (n, stride, w, h, dense) == (len(xyz), 132, 50, 30, False)
    got = out.download_fpfh().points["histogram"]
    raw = got.view(np.uint32)
    assert (raw[want_nan] == 0x7fc00000).all()                   # the quiet NaN, 33 times
    _check_fpfh(got, ref, "non-finite")
    spfh = dc.spfh(normals, 10)
    assert (spfh[want_nan] == 0).all()
    np.testing.assert_array_equal(spfh[~ref.fragile], ref.spfh[~ref.fragile])
    # a neighbour of a record with a NaN normal skips that pair: fewer than k - 1 pairs counted, on the GPU as in the reference
    short = ~want_nan & (ref.valid.sum(axis=1) < 9)
    assert short.sum() >= 30
    assert (np.abs(spfh[short].reshape(-1, 3, 11).astype(np.float64).sum(axis=2) - 100.0) > 1.0).all()
    # nothing non-finite: is_dense is the input's
    x2, d2c, n2, _ = _case(api, ctx, "uniform")
    assert d2c.fpfh_cloud(n2, 10).info() == (len(x2), 132, len(x2), 1, True)
    loose = api.DeviceCloud(_cloud(x2, width=30, height=50, is_dense=False), ctx=ctx)
    assert loose.fpfh_cloud(n2, 10).info() == (len(x2), 132, 30, 50, False)


def _unit(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    return (u / np.linalg.norm(u, axis=1)[:, None]).astype(np.float32)


def test_sizes(api, ctx):
    """n = k = 2 (hand-made normals: two records have no normal of their own) and n = k = 64."""
    for k in (2, 64):
        xyz = K.tiny(k)
        dc = api.DeviceCloud(_cloud(xyz), ctx=ctx)
        nrm = _unit(k, k) if k == 2 else _xyz3(dc.normals_cloud(10).download_normals().points)
        ref = F.fpfh(xyz, nrm, k)
        got = dc.fpfh(_normal_cloud(api, nrm), k)
        _check_fpfh(got, ref, "n = k = %d" % k)
        np.testing.assert_array_equal(dc.spfh(nrm, k)[~ref.fragile], ref.spfh[~ref.fragile])   # (an (n, 3) array: 12-byte normal records)
        assert (~ref.fragile_nb).sum() >= k // 2


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
    assert L.rsreg_cloud_fpfh(ctx.h, dc.h, nd.h, 1, out.h) == inv
    assert L.rsreg_cloud_fpfh(ctx.h, dc.h, nd.h, 65, out.h) == inv
    assert L.rsreg_cloud_fpfh(ctx.h, dc.h, nd.h, 41, out.h) == inv                  # n = k - 1
    assert L.rsreg_cloud_fpfh(ctx.h, dc.h, nd.h, 10, dc.h) == inv                   # out == in
    assert L.rsreg_cloud_fpfh(ctx.h, dc.h, nd.h, 10, nd.h) == inv                   # out == normals
    assert L.rsreg_cloud_fpfh(ctx.h, dc.h, nd.h, 10, None) == inv
    assert L.rsreg_cloud_fpfh(ctx.h, dc.h, None, 10, out.h) == inv
    short = api.DeviceCloud(_normal_cloud(api, _unit(39, 1)), ctx=ctx)              # normals of n - 1 records
    assert L.rsreg_cloud_fpfh(ctx.h, dc.h, short.h, 10, out.h) == inv
    assert L.rsreg_cloud_spfh(ctx.h, dc.h, short.h, 10, host.ctypes.data) == inv
    assert L.rsreg_cloud_spfh(ctx.h, dc.h, nd.h, 1, host.ctypes.data) == inv
    assert L.rsreg_cloud_spfh(ctx.h, dc.h, nd.h, 65, host.ctypes.data) == inv
    assert L.rsreg_cloud_spfh(ctx.h, dc.h, nd.h, 10, None) == inv
    holes = xyz.copy()
    holes[:5] = np.nan
    hc = api.DeviceCloud(_cloud(holes), ctx=ctx)
    assert L.rsreg_cloud_fpfh(ctx.h, hc.h, nd.h, 36, out.h) == inv                  # 35 finite records
    other = api.Context(0)
    foreign = api.DeviceCloud(_normal_cloud(api, _unit(40, 2)), ctx=other)
    assert L.rsreg_cloud_fpfh(ctx.h, dc.h, foreign.h, 10, out.h) == inv             # normals of another context
    assert out.download().points.tobytes() == before and out.stamp == stamp and (host == 0).all()
    with pytest.raises(lib.RsregError) as e:
        dc.fpfh(nd, 1)
    assert e.value.status == inv
    fe = api.FPFHEstimation()
    with pytest.raises(lib.RsregError) as e:
        fe.setRadiusSearch(0.05)
    assert e.value.status == inv and "not built" in str(e.value)
    lib.check(L.rsreg_cloud_fpfh(ctx.h, hc.h, nd.h, 35, out.h), ctx.h)              # exactly k finite records
    assert out.stamp[1] != stamp[1] and out.info()[:2] == (40, 132)
    assert L.rsreg_version() == 4


def test_grid_stride_loop(api, ctx):
    """66 000 records: more than the 65 536 workgroups of either launch.  2 000 sampled records, and the SPFH of their
    neighbours, against the reference."""
    xyz, dc, nd, nrm = _case(api, ctx, "many")
    k = 4
    ref = _ref(api, ctx, "many", k)
    got, spfh = dc.fpfh(nd, k), dc.spfh(nd, k)
    rng = np.random.default_rng(21)
    rows = np.concatenate([rng.choice(len(xyz), 1994, replace=False), [0, 1, 65535, 65536, 65999, 65998]])
    ok = rows[~ref.fragile_nb[rows]]
    assert len(ok) >= 1900
    assert got[ok].tobytes() == ref.fpfh[ok].tobytes()
    nb = np.unique(ref.idx[ok])
    nb = nb[~ref.fragile[nb]]
    np.testing.assert_array_equal(spfh[nb], ref.spfh[nb])
    assert F.blocks_ok(got).all()


def test_determinism(api, ctx):
    xyz, dc, nd, nrm = _case(api, ctx, "corner")
    first = dc.fpfh_cloud(nd, 10).download_fpfh().points.tobytes()
    assert dc.fpfh_cloud(nd, 10).download_fpfh().points.tobytes() == first          # a second call
    other = api.Context(0)                                                          # a fresh context that first indexed another cloud
    sph = api.DeviceCloud(_cloud(K.cloud("sphere")), ctx=other)
    sph.fpfh(sph.normals_cloud(10), 50)
    there = api.DeviceCloud(_cloud(xyz, seed=5), ctx=other)
    assert there.fpfh_cloud(_normal_cloud(api, nrm), 10).download_fpfh().points.tobytes() == first
    r16 = np.zeros((len(xyz), 4), np.float32)                                       # 16-byte records instead of 32-byte ones
    r16[:, :3] = xyz
    r16[:, 3] = 7.0
    rec16 = r16.view(np.dtype((np.void, 16))).reshape(-1)
    narrow = api.DeviceCloud(api.NormalCloud(rec16, len(rec16), 1, True), ctx=ctx)
    assert narrow.info()[1] == 16
    assert narrow.fpfh_cloud(nd, 10).download_fpfh().points.tobytes() == first
    fe = api.FPFHEstimation()                                                       # the PCL-style class, device and host input
    fe.setInputCloud(dc)
    fe.setInputNormals(nd)
    fe.setKSearch(10)
    assert fe.getKSearch() == 10 and fe.compute().download_fpfh().points.tobytes() == first
    fe.setInputCloud(_cloud(xyz))
    fe.setInputNormals(_normal_cloud(api, nrm))
    host = fe.compute()
    assert host.points.tobytes() == first and (host.width, host.height, host.is_dense) == (len(xyz), 1, True)


def test_cpp_adaptor(api, ctx, tmp_path):
    """tests/cpp/fpfh_runner.cpp (rsreg::NormalEstimation -> rsreg::FPFHEstimation) gives the bytes of the Python path, from host
    clouds and from device clouds."""
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "fpfh_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fpfh_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    xyz, _ = K.holes()
    cloud = _cloud(xyz, width=50, height=30, is_dense=False)
    dc = api.DeviceCloud(cloud, ctx=ctx)
    want = dc.fpfh_cloud(dc.normals_cloud(12), 16).download_fpfh()
    cloud.points.tofile(str(tmp_path / "in.bin"))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), "50", "30", "12", "16", str(tmp_path / "host.bin"), str(tmp_path / "dev.bin")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    vals = dict(l.split() for l in r.stdout.strip().splitlines())
    for name in ("host.bin", "dev.bin"):
        assert open(str(tmp_path / name), "rb").read() == want.points.tobytes()
    assert int(vals["size"]) == int(vals["size_device"]) == len(xyz) and (int(vals["width"]), int(vals["height"])) == (50, 30)
    assert vals["dense"] == vals["dense_device"] == "0" and vals["k"] == "16" and vals["radius_refused"] == "1"
    assert not want.is_dense
