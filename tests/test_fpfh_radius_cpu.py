"""The numpy reference of FPFHEstimationOMP by radius (tests/fpfh_radius_ref.py) against hand-computed values and its own invariants,
and the CONDITIONS tests/test_fpfh_radius_gpu.py puts on its inputs, checked on every case.  No GPU: what is checked here is the
yardstick, not the engine."""
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


def _differing(a, b):
    """values that differ between two results, a NaN on both sides counted as equal"""
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())


def test_hand_computed_pair():
    """The pair of tests/test_fpfh_cpu.py, one unit apart, bins 6, 5 and 2 from either side.  radius 1.5: m = 2, hist_incr = 100,
    each block holds one 100; the FPFH of each record is the other's SPFH times 1 / d2 = 1, normalised.  radius 1: the other record
    lies AT the radius and is no neighbour -- m = 1, no addition, zeros."""
    xyz = np.float32([[0, 0, 0], [1, 0, 0]])
    nrm = np.float32([[0, 0, 1], [0.6, 0, 0.8]])
    r = FR.fpfh_radius(xyz, nrm, 1.5)
    want = np.zeros(33, np.float32)
    want[[6, 11 + 5, 22 + 2]] = 100.0
    assert r.m.tolist() == [2, 2] and r.I.tolist() == [0, 0, 1, 1] and r.J.tolist() == [0, 1, 0, 1]
    assert (r.spfh == want).all() and (r.fpfh == want).all() and r.valid.tolist() == [False, True, True, False]
    assert not r.fragile.any() and not r.nan_rows.any()
    r = FR.fpfh_radius(xyz, nrm, 1.0)
    assert r.m.tolist() == [1, 1] and (r.spfh == 0).all() and (r.fpfh == 0).all()


def test_table_is_the_sequential_sum():
    """m = 4: hist_incr = 100 / 3 in float32; three pairs in one bin give ((incr + incr) + incr), not 100."""
    third = np.float32(100.0) / np.float32(3.0)
    counts = np.array([[0, 1, 2, 3]])
    rows = FR.spfh_rows(counts, np.array([4], np.uint32))
    assert rows.dtype == np.float32
    assert rows[0].tolist() == [0.0, third, np.float32(third + third), np.float32(np.float32(third + third) + third)]
    # m = 300: the 299th partial sum, one float addition after the other
    incr = np.float32(100.0) / np.float32(299.0)
    acc = np.float32(0.0)
    for _ in range(299):
        acc = np.float32(acc + incr)
    assert FR.spfh_rows(np.array([[299]]), np.array([300], np.uint32))[0, 0] == acc
    assert (FR.spfh_rows(np.array([[0]]), np.array([1], np.uint32)) == 0).all()       # m = 1: nothing is divided by zero


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_conditions_and_invariants(name):
    """On every case: m is radius_ref's count; every counted pair is counted once per feature; every row without a NaN has blocks
    that sum to 100 or are zero; and the CONDITIONS of the GPU test hold on the reference alone -- at most 1 % fragile records, at
    most 5 % fragile or beside a fragile one, at most 1 value in 10 000 moved by running the float64 sums the other way round."""
    xyz, nrm, radius = C.case(name)
    r, d = C.ref(name), C.ref(name, "descending")
    assert (r.m == R.counts(xyz, radius)).all()
    pairs = np.bincount(r.I[r.valid], minlength=len(xyz))
    assert (r.counts.reshape(-1, 3, 11).sum(axis=2) == pairs[:, None]).all() and (pairs <= np.maximum(r.m, 1) - 1).all()
    clean = ~np.isnan(r.fpfh).any(axis=1)
    assert F.blocks_ok(r.fpfh[clean]).all()
    full = clean & (pairs == r.m.astype(np.int64) - 1) & (r.m > 1)
    assert np.abs(r.spfh[full].reshape(-1, 3, 11).astype(np.float64).sum(axis=2) - 100.0).max() <= 1e-2 * max(1, r.m.max() / 64)
    assert (r.spfh[r.nan_rows] == 0).all() and np.isnan(r.fpfh[r.nan_rows]).all()
    assert (r.spfh.tobytes() == d.spfh.tobytes()) and (np.isnan(r.fpfh) == np.isnan(d.fpfh)).all()
    differ = _differing(r.fpfh, d.fpfh)
    print("%s: n %d, m <= %d, largest bin count %d, fragile %d, fragile or beside one %d, values the order moves %d of %d" %
          (name, len(xyz), r.m.max(), r.counts.max(), r.fragile.sum(), r.fragile_nb.sum(), differ, r.fpfh.size))
    assert r.fragile.mean() <= C.FRAGILE_CAP and r.fragile_nb.mean() <= C.FRAGILE_NB_CAP
    assert differ <= C.DIFFER_CAP * r.fpfh.size
    both = ~np.isnan(r.fpfh)
    assert (FR.ulp_apart(r.fpfh[both], d.fpfh[both]) <= 1).all()


def test_what_the_cases_are_for():
    """Each case reaches what it is named for."""
    r = C.ref("corner_0.12")
    assert r.m.max() > 64 and r.counts.max() > 63                       # past the k-search's 64-entry table and one 64-point read
    assert C.ref("corner_0.25").m.max() > 256
    r = C.ref("uniform_0.12")
    assert (r.m == 1).sum() >= 10 and (r.m == 2).sum() >= 10
    assert (r.spfh[r.m == 1] == 0).all() and (r.fpfh[r.m == 1] == 0).all()
    two = np.flatnonzero(r.m == 2)
    assert np.isin(r.spfh[two], [0.0, 100.0]).all() and (r.spfh[two].sum(axis=1) == 300.0).all()
    # exact copies: counted in m, skipped in both passes
    r = C.ref("copies_0.12")
    base = C.ref("uniform_0.12")
    stack = [7] + list(range(1500, 1512))
    assert (r.m[stack] == base.m[7] + 12).all() and r.m[100] == base.m[100] + 3
    assert len({r.fpfh[i].tobytes() for i in stack}) == 1 and len({r.spfh[i].tobytes() for i in stack}) == 1
    r = C.ref("pile")
    assert (r.m[-13:] == 13).all() and (r.spfh[-13:] == 0).all() and (r.fpfh[-13:] == 0).all() and not r.nan_rows.any()
    # non-finite records and normals: zero SPFH rows that still sit in their neighbours' sums, NaN FPFH rows
    xyz, nrm, radius = C.case("holes")
    r = C.ref("holes")
    bad_normal = np.isfinite(xyz).all(axis=1) & ~np.isfinite(nrm).all(axis=1)
    assert r.nan_rows.sum() == 70 and bad_normal.sum() == C.HOLES_BAD_NORMALS and (r.m[bad_normal] >= 1).all()
    assert (r.m[~np.isfinite(xyz).all(axis=1)] == 0).all()
    beside = np.unique(r.I[bad_normal[r.J] & (r.I != r.J)])
    beside = beside[~r.nan_rows[beside]]
    assert len(beside) >= 30 and np.isfinite(r.fpfh[beside]).all()
    r = C.ref("radius_normals")
    assert 20 <= r.nan_rows.sum() <= 300 and (r.m[r.nan_rows] >= 1).all()
    # a record AT the radius is no neighbour: an inner record of the lattice has its 3 x 3 x 3 block and nothing else
    xyz, _, radius = C.case("at_the_radius")
    r = C.ref("at_the_radius")
    inner = (6 * 12 + 6) * 12 + 6
    assert r.m[inner] == 27 and r.m.max() == 27 and R.r2_f32(radius) == np.float32(4.0 * K.H * K.H)
    assert R.counts(xyz, np.nextafter(np.float32(radius), np.float32(1.0)))[inner] == 33
    # a denormal d2: w = +inf, the rows of the two records are NaN by the arithmetic alone
    r = C.ref("denormal")
    pair = r.d2[(r.I >= 1500) & (r.I != r.J)]
    assert len(pair) == 2 and (pair == np.float32(2.0 ** -140)).all() and (pair > 0).all()
    assert not r.nan_rows.any() and np.isnan(r.fpfh[-2:]).all() and not np.isnan(r.fpfh[:-2]).any()
    assert (r.spfh[-2:].sum(axis=1) == 300.0).all()
    r = C.ref("many")
    assert len(r.m) > 65536 and 2.0 <= r.m.mean() <= 5.0


def test_invariant_under_a_permutation_of_the_records():
    """The rows go with the records: SPFH and counts exactly; FPFH within one float32 step, because the float64 sums run in another
    order (and then at most 1 value in 10 000 moves)."""
    xyz, nrm, radius = C.case("corner_0.12")
    r = C.ref("corner_0.12")
    perm = np.random.default_rng(41).permutation(len(xyz))
    p = FR.fpfh_radius(xyz[perm], nrm[perm], radius)
    assert (p.m == r.m[perm]).all() and p.spfh.tobytes() == r.spfh[perm].tobytes()
    assert (FR.ulp_apart(p.fpfh, r.fpfh[perm]) <= 1).all()
    assert _differing(p.fpfh, np.ascontiguousarray(r.fpfh[perm])) <= C.DIFFER_CAP * r.fpfh.size


def test_exports_and_the_python_class_refuse_without_a_device():
    """The library exports the two entry points; api.FPFHEstimationOMP refuses both searches and neither before any device call, and
    api.FPFHEstimation still refuses a radius."""
    from rsreg_amd import api, lib
    handle = lib.lib()
    assert handle.rsreg_cloud_fpfh_radius is not None and handle.rsreg_cloud_spfh_radius is not None
    fe = api.FPFHEstimationOMP()
    fe.setInputCloud(object())
    fe.setInputNormals(object())
    with pytest.raises(lib.RsregError, match="neither") as e:
        fe.compute()
    assert e.value.status == lib.RSREG_ERR_INVALID_ARG
    fe.setKSearch(10)
    fe.setRadiusSearch(0.05)
    fe.setNumberOfThreads(8)
    assert fe.getKSearch() == 10 and fe.getRadiusSearch() == 0.05
    with pytest.raises(lib.RsregError, match="both") as e:
        fe.compute()
    assert e.value.status == lib.RSREG_ERR_INVALID_ARG
    fe.setKSearch(0)
    fe.setRadiusSearch(0)
    with pytest.raises(lib.RsregError, match="neither"):
        fe.compute()
    with pytest.raises(lib.RsregError, match="not built"):
        api.FPFHEstimation().setRadiusSearch(0.05)


def test_cpp_adaptor_refuses_both_searches_and_neither():
    """tests/cpp/fpfh_radius_runner.cpp compiles with a host compiler, and its `refuse` mode sees rsreg::FPFHEstimationOMP throw
    RSREG_ERR_INVALID_ARG for both searches and for neither without a device."""
    from rsreg_amd import lib
    lib.build()
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "fpfh_radius_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fpfh_radius_runner.cpp"),
                        "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe, "refuse"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "refused yes", r.stdout
