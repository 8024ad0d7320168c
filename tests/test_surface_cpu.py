"""The numpy reference of the search-surface calls (tests/surface_ref.py) against a brute force, against the in-cloud references it
must reproduce when the queries ARE the surface, and against hand-computed values; and the CONDITIONS tests/test_surface_gpu.py
puts on its inputs, checked on every case.  No GPU: what is checked here is the yardstick, not the engine."""
import os
import re

import numpy as np
import pytest

import fpfh_cases as K
import fpfh_radius_cases as C
import fpfh_ref as F
import radius_ref as R
import surface_cases as SC
import surface_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _differing(a, b):
    """values that differ between two results, a NaN on both sides counted as equal"""
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())


@pytest.mark.parametrize("name,pick", SC.CASES, ids=SC.IDS)
def test_conditions_on_the_cases(name, pick):
    """The conditions of surface_cases' docstring on the reference alone, each figure printed; and what every case is built to hold."""
    q, s, nrm, radius = SC.case(name, pick)
    r, d = SC.ref(name, pick), SC.ref(name, pick, "descending")
    fin = np.isfinite(q).all(axis=1)
    moved = _differing(r.fpfh, d.fpfh)
    share = r.needed.mean()
    print("%s 1/%d: queries %d (%d not finite), m %d .. %d, needed %d of %d (%.1f %%), with a fragile neighbour %.2f %%, values the order moves %d of %d"
          % (name, pick, len(q), int((~fin).sum()), r.m[fin].min(), r.m.max(), int(r.needed.sum()), len(s), 100 * share, 100 * r.fragile_nb.mean(), moved,
             r.fpfh.size))
    assert r.fragile_nb.mean() <= SC.FRAGILE_NB_CAP
    assert moved <= SC.DIFFER_CAP * r.fpfh.size
    assert share < SC.NEEDED_CAP or (name, pick) not in SC.SUBSET
    assert (r.m[-2:] == 0).all() and np.isnan(r.fpfh[-2:]).all()              # the two far queries
    assert (r.m[-7:-2] >= 1).all()                                            # the exact surface records find themselves
    assert (r.m[~fin] == 0).all() and np.isnan(r.fpfh[~fin]).all()
    assert (np.isnan(r.fpfh).any(axis=1) == r.nan_rows).all()
    assert F.blocks_ok(r.fpfh[~r.nan_rows]).all()
    assert (r.spfh[~r.needed] == 0).all()
    if name == "corner_0.12":
        assert r.m.max() > 64                                                 # past one 64-point read
    if name == "holes":
        assert (~fin).any() and (~np.isfinite(s).all(axis=1)).any() and (~np.isfinite(nrm).all(axis=1)).any()
    n = SC.ref_normals(name, pick)
    assert (n.m == r.m).all() and (n.valid == (fin & (r.m >= 3))).all()


def test_tree_candidates_against_brute_force():
    q, s, _, radius = SC.case("holes", 20)
    a, b = SR.search(q, s, radius), SR.search(q, s, radius, brute=True)
    assert (a.off == b.off).all() and (a.idx == b.idx).all() and (a.I == b.I).all() and a.counts().sum() > 100
    # ... and at a radius that puts lattice records AT it: 1.5 H around a point half a step off the lattice
    lat = K.lattice()
    query = (lat[5 * 144 + 5 * 12 + 5] + np.float32([K.H / 2, 0, 0]))[None]
    for radius in (1.5 * K.H, float(np.nextafter(np.float32(1.5 * K.H), np.float32(1)))):
        a, b = SR.search(query, lat, radius), SR.search(query, lat, radius, brute=True)
        assert (a.idx == b.idx).all()


def test_lattice_by_hand():
    """The 12^3 lattice of step H = 2^-6 and an inner lattice point moved by H / 2 along x.  Offsets are (+-0.5 | +-1.5, 0 | +-1,
    0 | +-1) H and on: d2 / H^2 = 0.25 + {0, 1, 2} for the eight-plus-two nearest columns, 2.25 for the two at +-1.5 H along x and
    for the eight at (+-0.5, +-1, +-1).  At r = 1.5 H, r2 = 2.25 H^2 exactly: 2 + 8 = 10 neighbours, the ten AT the radius are not.
    At the next float above 1.5 H they are: 20."""
    lat = K.lattice()
    query = (lat[5 * 144 + 5 * 12 + 5] + np.float32([K.H / 2, 0, 0]))[None]
    assert SR.counts(query, lat, 1.5 * K.H).tolist() == [10]
    up = float(np.nextafter(np.float32(1.5 * K.H), np.float32(1)))
    assert SR.counts(query, lat, up).tolist() == [20]


@pytest.mark.parametrize("name", ["corner_0.12", "holes", "pile"])
def test_queries_equal_to_the_surface_reproduce_the_in_cloud_references(name):
    xyz, nrm, radius = C.case(name)
    nb = SR.search(xyz, xyz, radius)
    assert (nb.counts() == R.counts(xyz, radius)).all()
    own = R.normals(xyz, radius)
    got = SR.normals(xyz, xyz, radius, nb=nb)
    assert (got.valid == own.valid).all()
    assert got.normal.tobytes() == own.normal.tobytes() and got.curvature.tobytes() == own.curvature.tobytes()
    base = C.ref(name)
    r = SR.fpfh(xyz, xyz, nrm, radius, nb=nb, surface_ref=base)
    assert r.needed.tolist() == np.isfinite(xyz).all(axis=1).tolist() and r.spfh.tobytes() == base.spfh.tobytes()
    rows = np.isfinite(nrm).all(axis=1) & np.isfinite(xyz).all(axis=1)       # the in-cloud NaN rule for a record's own normal is not here
    assert rows.sum() > 0 and r.fpfh[rows].tobytes() == base.fpfh[rows].tobytes()
    assert (r.m == base.m).all()
    if name == "pile":                                                        # twelve copies and nothing else in range: zeros, not NaN
        assert (r.m[-13:] == 13).all() and (r.fpfh[-13:].view(np.uint32) == 0).all()


def test_no_neighbour_is_nan_and_coincident_is_zero():
    s = np.float32([[0, 0, 0], [0, 0, 0], [1, 0, 0]])
    nrm = np.float32([[0, 0, 1], [0, 0, 1], [0.6, 0, 0.8]])
    q = np.float32([[0, 0, 0], [5, 5, 5], [np.nan, 0, 0]])
    r = SR.fpfh(q, s, nrm, 0.5)
    assert r.m.tolist() == [2, 0, 0] and r.needed.tolist() == [True, True, False]
    assert (r.fpfh[0].view(np.uint32) == 0).all() and np.isnan(r.fpfh[1:]).all() and r.nan_rows.tolist() == [False, True, True]
    n = SR.normals(q, s, 0.5)
    assert np.isnan(n.normal).all() and not n.valid.any()                     # m < 3 everywhere


def test_header_and_package_name_the_calls(rs):
    """The four calls are declared in the header and listed among the exports (tests/test_abi.py checks that the two agree)."""
    from rsreg_amd import lib
    hdr = open(os.path.join(ROOT, "include", "rsreg.h")).read()
    for name in ("rsreg_cloud_radius_count_surface", "rsreg_cloud_normals_radius_surface", "rsreg_cloud_fpfh_radius_surface",
                 "rsreg_cloud_spfh_radius_surface"):
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M) and name in lib.EXPORTS
    from rsreg_amd import api
    est = api.FPFHEstimationOMP()
    est.setSearchSurface(None)
    with pytest.raises(lib.RsregError):
        api.FPFHEstimation().setSearchSurface(object())
