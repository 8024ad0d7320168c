"""CPU: the reference of PassThrough / StatisticalOutlierRemoval (tests/sor_ref.py) against itself and against cases worked out
by hand, and the build: the library exports the three new entry points and hipcc compiles csrc/filters.hip for gfx950."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sor_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 2.0 ** -6


def lattice(m):
    """m^3 points on a lattice of spacing H = 2^-6 around (0, 0, 1): every difference, square and sum is exact in float32."""
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)
    return (g * H + np.array([0.0, 0.0, 1.0])).astype(np.float32), g


@pytest.mark.parametrize("n,k,seed", [(2000, 1, 1), (3000, 8, 2), (4000, 50, 3), (2500, 64, 4)])
def test_tree_path_equals_brute_force(n, k, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.random((n, 3)).astype(np.float32)
    xyz[:, 2] *= 0.05                                  # (a slab: neighbourhoods of very different sizes)
    xyz[rng.integers(0, n, n // 10)] = xyz[rng.integers(0, n, n // 10)]   # exact copies
    xyz[5], xyz[77] = np.nan, np.inf
    a = S.knn_mean_distance(xyz, k, "brute")
    b = S.knn_mean_distance(xyz, k, "tree")
    assert (a.view(np.uint32) == b.view(np.uint32)).all()
    assert a[5] == 0 and a[77] == 0


def test_lattice_by_hand():
    xyz, g = lattice(6)
    d = S.knn_mean_distance(xyz, 6)
    inner = ((g > 0) & (g < 5)).all(axis=1)
    assert (d[inner] == np.float32(H)).all()            # six neighbours at H
    corner = np.flatnonzero((g == 0).all(axis=1))[0]
    r2 = float(np.sqrt(np.float32(2 * H * H)))           # three at H, three at sqrt(2) H
    want = np.float32((((((H + H) + H) + r2) + r2) + r2) / 6.0)
    assert d[corner] == want
    # both paths of the reference, and the statistics in closed form for the inner points alone
    assert (S.knn_mean_distance(xyz, 6, "tree").view(np.uint32) == d.view(np.uint32)).all()
    n_valid, mean, stddev, thr = S.sor_stats(xyz[inner], np.full(int(inner.sum()), H, np.float32), 1.5)
    assert (n_valid, mean, stddev, thr) == (64, H, 0.0, H)


def test_mean_k_one_is_the_nearest_other_point():
    rng = np.random.default_rng(11)
    xyz = rng.random((300, 3)).astype(np.float32)
    d = S.knn_mean_distance(xyz, 1)
    for i in range(len(xyz)):
        d2 = sorted(float(S.d2_f32(xyz[i], xyz[j])) for j in range(len(xyz)))
        assert d[i] == np.sqrt(np.float32(d2[1]))


def test_cloud_of_copies():
    rng = np.random.default_rng(12)
    base = rng.random((200, 3)).astype(np.float32)
    xyz = np.repeat(base, 3, axis=0)
    keep, d, (n_valid, mean, stddev, thr) = S.sor(xyz, 2, 1.0)
    assert (d == 0).all() and (mean, stddev, thr) == (0.0, 0.0, 0.0) and keep.all() and n_valid == 600
    d3 = S.knn_mean_distance(xyz, 3)                     # the third neighbour is the nearest OTHER point
    nearest = S.knn_mean_distance(base, 1)
    assert (d3 == (np.repeat(nearest, 3).astype(np.float64) / 3.0).astype(np.float32)).all()


def test_non_finite_records_and_negative():
    xyz, _ = lattice(4)
    xyz = np.concatenate([xyz, np.array([[0.5, 0.5, 3.0]], np.float32)])   # one far outlier
    xyz[3] = np.nan
    xyz[10, 1] = np.inf
    keep, d, st = S.sor(xyz, 6, 1.0)
    assert d[3] == 0 and d[10] == 0 and st[0] == len(xyz) - 2
    assert keep[3] and keep[10] and not keep[-1]
    nkeep, _, _ = S.sor(xyz, 6, 1.0, negative=True)
    assert not nkeep[3] and not nkeep[10] and nkeep[-1]
    fin = S.finite_rows(xyz)
    assert (nkeep[fin] == ~keep[fin]).all()


def test_error_cases():
    xyz, _ = lattice(2)                                   # 8 points
    with pytest.raises(ValueError):
        S.knn_mean_distance(xyz, 8)                       # needs 9 finite records
    S.knn_mean_distance(xyz, 7)
    bad = xyz.copy()
    bad[0] = np.nan
    with pytest.raises(ValueError):
        S.knn_mean_distance(bad, 7)
    one = np.array([[0, 0, 1], [np.nan, 0, 0]], np.float32)
    with pytest.raises(ValueError):
        S.sor_stats(one, np.zeros(2, np.float32), 1.0)


def test_passthrough_reference():
    xyz = np.array([[0, 0, 0.2], [0, 0, 0.1], [0, 0, 2.5], [0, 0, 2.6], [np.nan, 0, 1.0], [0, np.inf, 1.0], [0, 0, 0.0]], np.float32)
    assert S.passthrough_keep(xyz, 2, 0.2, 2.5).tolist() == [True, False, True, False, False, False, False]
    assert S.passthrough_keep(xyz, 2, 0.2, 2.5, negative=True).tolist() == [False, True, False, True, False, False, True]
    assert S.passthrough_keep(xyz, 2).tolist() == [True, True, True, True, False, False, False]   # FLT_MIN .. FLT_MAX: z = 0 is out


def test_library_exports_the_filters(rs):
    from rsreg_amd import lib
    lib.build()
    handle = lib.lib()
    for name in ("rsreg_cloud_passthrough", "rsreg_cloud_sor", "rsreg_cloud_knn_mean_distance"):
        assert name in lib.EXPORTS and getattr(handle, name) is not None
    assert C.sizeof(lib.SorStats) == 40
    assert "filters.hip" in lib.SOURCES and "knn_kernels.hpp" in lib.HEADERS
    from rsreg_amd import PassThrough, StatisticalOutlierRemoval, api
    assert PassThrough is api.PassThrough and StatisticalOutlierRemoval is api.StatisticalOutlierRemoval
    assert hasattr(api.DeviceCloud, "knn_mean_distance")
    sor = StatisticalOutlierRemoval()
    assert (sor.mean_k, sor.stddev_mult) == (1, 0.0)      # PCL's defaults
    p = PassThrough()
    assert (np.float32(p.lo), np.float32(p.hi)) == (S.FLT_MIN, S.FLT_MAX)


def test_hipcc_compiles_filters_for_gfx950(rs, tmp_path):
    from rsreg_amd import lib
    src = os.path.join(lib.CSRC, "filters.hip")
    assert os.path.exists(src)
    obj = str(tmp_path / "filters.o")
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *lib._flags(False), "-c", src, "-o", obj],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert os.path.getsize(obj) > 0


def test_cpp_adaptor_compiles(tmp_path):
    """tests/cpp/sor_runner.cpp -- the reference's pre-filter sequence against rsreg:: -- compiles with a host compiler."""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sor_runner.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
