"""CPU: the reference of the k-NN search with indices and of NormalEstimation (tests/normals_ref.py) on inputs whose answer is
known in closed form, its two search paths against each other, and the build: the library exports rsreg_cloud_knn and
rsreg_cloud_normals, the Python layer has the adaptors, and the C++ runner compiles."""
import os
import subprocess

import numpy as np
import pytest

import normals_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 2.0 ** -6


def lattice(m, mz=None):
    """m x m x mz points on a lattice of spacing H = 2^-6 around (0, 0, 1): every difference, square and sum is exact."""
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m if mz is None else mz), indexing="ij"), -1).reshape(-1, 3)
    return (g * H + np.array([0.0, 0.0, 1.0])).astype(np.float32), g


def test_exact_lattice_plane():
    """One layer of the lattice: every neighbourhood lies in z = 1, so the covariance has an exactly zero row and column --
    the normal is +-z exactly, towards the origin -z, and the curvature 0."""
    xyz, _ = lattice(9, 1)
    for k in (5, 9, 25):
        r = N.normals(xyz, k)
        assert (r.normal == np.array([0, 0, -1], np.float32)).all()
        assert (r.curvature == 0).all() and (r.evals[:, 0] == 0).all()
        up = N.normals(xyz, k, viewpoint=(0.0, 0.0, 5.0))
        assert (up.normal == np.array([0, 0, 1], np.float32)).all()


def test_sphere_gives_the_radial_direction():
    """Points on a sphere of radius R around c, seen from c: the normal of a cap of angular radius a is the axis of the cap
    up to the asymmetry of the sample; the angle to the radial direction through the record stays below the cap's own
    angular radius a = asin(dmax / R) by a wide margin (bound used: a), and the normal points at the viewpoint c."""
    rng = np.random.default_rng(1)
    u = rng.standard_normal((4000, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    c, R = np.array([0.1, -0.2, 1.5]), 0.5
    xyz = (c + R * u).astype(np.float32)
    r = N.normals(xyz, 12, viewpoint=c)
    radial = (c - xyz.astype(np.float64))
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    cosang = (r.normal.astype(np.float64) * radial).sum(axis=1)
    a = np.arcsin(np.sqrt(r.d2[:, -1].astype(np.float64)) / R)
    assert (cosang > 0).all()
    assert (np.arccos(np.clip(cosang, -1, 1)) <= a).all()
    assert (r.curvature < 0.05).all()


def test_tie_rule_on_a_lattice():
    xyz, g = lattice(5)
    idx, d2 = N.knn(xyz, 7)
    centre = np.flatnonzero((g == 2).all(axis=1))[0]
    want = sorted([centre] + [np.flatnonzero((g == np.array([2, 2, 2]) + e).all(axis=1))[0]
                              for e in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1])])
    assert idx[centre, 0] == centre and sorted(idx[centre]) == want
    assert (idx[centre, 1:] == np.sort(idx[centre, 1:])).all() and (d2[centre] == np.float32([0] + [H * H] * 6)).all()
    # k = 4: three of the six neighbours at H -- the three with the lowest indices
    idx4, _ = N.knn(xyz, 4)
    assert idx4[centre].tolist() == [centre] + sorted(want[i] for i in range(7) if want[i] != centre)[:3]
    # copies of a record: all at distance 0, lowest indices first, whichever copy asks
    xyz2 = np.concatenate([xyz, np.repeat(xyz[centre][None], 5, axis=0)])
    idx2, d22 = N.knn(xyz2, 3)
    for i in [centre] + list(range(len(xyz), len(xyz) + 5)):
        assert idx2[i].tolist() == [centre, len(xyz), len(xyz) + 1] and (d22[i] == 0).all()
    # a record that is not finite: row -1 / 0, and nobody's neighbour
    xyz2[3] = np.nan
    idx3, d23 = N.knn(xyz2, 7)
    assert (idx3[3] == -1).all() and (d23[3] == 0).all() and not (idx3[np.arange(len(xyz2)) != 3] == 3).any()
    with pytest.raises(ValueError):
        N.knn(xyz2[:6], 6)                                  # five finite records


@pytest.mark.parametrize("n,k,seed", [(1500, 1, 1), (2500, 10, 2), (2000, 64, 3)])
def test_tree_path_equals_brute_force(n, k, seed):
    rng = np.random.default_rng(seed)
    xyz = np.round(rng.random((n, 3)) * 32).astype(np.float32) / 32          # a coarse lattice: ties everywhere
    xyz[:, 2] *= 0.25
    xyz[rng.integers(0, n, n // 10)] = xyz[rng.integers(0, n, n // 10)]       # exact copies
    xyz[:80] = xyz[0]                                                         # a pile larger than k
    xyz[5], xyz[77] = np.nan, np.inf
    ia, da = N.knn(xyz, k, "brute")
    ib, db = N.knn(xyz, k, "tree")
    assert (ia == ib).all() and (da.view(np.uint32) == db.view(np.uint32)).all()
    assert (ia[5] == -1).all() and (da[77] == 0).all()


def test_coincident_neighbourhood_and_non_finite():
    xyz = np.array([[0.5, 0.25, 1.0]] * 4 + [[np.nan, 0, 0]] + [[3, 3, 3], [3, 3, 3.5], [3, 3.5, 3]], np.float32)
    r = N.normals(xyz, 3)
    assert (r.normal[:4] == np.array([0, 0, -1], np.float32)).all() and (r.curvature[:4] == 0).all()
    assert np.isnan(r.normal[4]).all() and np.isnan(r.curvature[4])
    assert abs(abs(r.normal[5, 0]) - 1) < 1e-6 and r.normal[5, 0] < 0        # the plane x = 3, seen from the origin


def test_library_exports_the_normals(rs):
    import ctypes as C

    from rsreg_amd import lib
    lib.build()
    handle = lib.lib()
    for name in ("rsreg_cloud_knn", "rsreg_cloud_normals"):
        assert name in lib.EXPORTS and getattr(handle, name) is not None
    assert "normals_kernels.hpp" in lib.HEADERS
    from rsreg_amd import NormalEstimation, api
    assert NormalEstimation is api.NormalEstimation and api.NORMAL_DTYPE.itemsize == 32
    assert hasattr(api.DeviceCloud, "knn") and hasattr(api.DeviceCloud, "normals")
    ne = NormalEstimation()
    ne.setKSearch(10)
    ne.setViewPoint(1, 2, 3)
    assert ne.getKSearch() == 10 and ne.getViewPoint() == (1.0, 2.0, 3.0)
    assert C.sizeof(C.c_int32) == 4


def test_cpp_runner_compiles(tmp_path):
    """tests/cpp/normals_runner.cpp -- NormalEstimation through rsreg:: on host and device clouds -- compiles with a host compiler."""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "normals_runner.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
