"""Inputs of the radius-FPFH tests (tests/test_fpfh_radius_cpu.py, tests/test_fpfh_radius_gpu.py): the clouds of fpfh_cases with a
radius, each case (xyz, normals, radius), float32, made once.  The normals are the reference's (tests/normals_ref.py at k = 10, or
tests/radius_ref.py where a case says so) or hand-made: the same arrays go to the reference and, uploaded, to the engine.

The caps below are CONDITIONS on the inputs, decided on the reference alone (tests/test_fpfh_radius_cpu.py checks every case):
at most 1 % of the records fragile, at most 5 % fragile or with a fragile neighbour, and at most 1 value in 10 000 that moves when
the float64 sums run in descending instead of ascending order.
"""
import functools

import numpy as np

import fpfh_cases as K

H = K.H
FRAGILE_CAP, FRAGILE_NB_CAP, DIFFER_CAP = 0.01, 0.05, 1e-4
PILE_AT = (3.0, 3.0, 3.0)
TINY = 2.0 ** -70            # a pair this far apart: d2 = 2^-140, a denormal float32, and 1.0f / d2 = +inf


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _unit(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    return (u / np.linalg.norm(u, axis=1)[:, None]).astype(np.float32)


def _k10(xyz):
    import normals_ref as N
    return np.ascontiguousarray(N.normals(xyz, 10).normal)


def _named(name, radius):
    return lambda: (K.cloud(name).copy(), K.ref_normals(name).copy(), radius)


def pile():
    """The uniform box and, far from it, one record with twelve exact copies: m = 13, nothing at a positive distance."""
    xyz = np.concatenate([K.uniform(), np.tile(np.float32(PILE_AT), (13, 1))]).astype(np.float32)
    return xyz, _k10(xyz), 0.12


def holes():
    """fpfh_cases.holes(): 40 records that are not finite, and 30 finite ones whose NORMAL is not (20 NaN, 10 with an inf)."""
    xyz, bad = K.holes()
    nrm = _k10(xyz)
    nrm[bad[:20]] = np.nan
    nrm[bad[20:], 2] = np.inf
    return xyz, nrm, 0.12


HOLES_BAD_NORMALS = 30
ENGINE_NORMALS_RADIUS = 0.12   # the uniform box: a few dozen records have fewer than three neighbours there and get NaN normals


def radius_normals():
    """The uniform box with the normals of NormalEstimation::setRadiusSearch(0.12) (the reference's here; the GPU test takes the
    engine's): the records with m < 3 have NaN normals."""
    import radius_ref as R
    xyz = K.uniform()
    return xyz, np.ascontiguousarray(R.normals(xyz, ENGINE_NORMALS_RADIUS).normal), 0.2


def at_the_radius():
    """The 12^3 lattice of spacing 2^-6 with radius = 2 * 2^-6 and hand-made normals: the records two steps along an axis lie AT the
    radius (d2 == r2 exactly in float32) and are not neighbours; an inner record has the 27 of its 3 x 3 x 3 block."""
    xyz = K.lattice()
    return xyz, _unit(len(xyz), 31), 2.0 * H


def denormal():
    """The uniform box and two records 2^-70 apart at the origin, 0.4 from the box: they are each other's only neighbour at a
    positive distance, d2 = 2^-140 is a denormal float32, w = +inf."""
    xyz = np.concatenate([K.uniform(), np.float32([[0.0, 0.0, 0.0], [TINY, 0.0, 0.0]])]).astype(np.float32)
    nrm = _k10(xyz)
    nrm[-2:] = np.float32([[0.0, 0.6, 0.8], [0.6, 0.0, 0.8]])
    return xyz, nrm, 0.12


def many():
    """66 000 records: more than the 65 536 workgroups of a launch, about three neighbours each."""
    xyz = K.many()
    return xyz, _unit(len(xyz), 32), 0.025


CASES = {
    "corner_0.05": _named("corner", 0.05),         # m up to about 20
    "corner_0.12": _named("corner", 0.12),         # bin counts above 63, neighbourhoods above 64: more than one 64-point read of a row
    "corner_0.25": _named("corner", 0.25),         # m in the hundreds
    "sphere_0.2": _named("sphere", 0.2),
    "uniform_0.12": _named("uniform", 0.12),       # records with m = 1 and with m = 2
    "copies_0.12": _named("copies", 0.12),
    "pile": pile,
    "holes": holes,
    "radius_normals": radius_normals,
    "at_the_radius": at_the_radius,
    "denormal": denormal,
    "many": many,
}


@functools.lru_cache(maxsize=None)
def case(name):
    xyz, nrm, radius = CASES[name]()
    return _frozen(np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(nrm, np.float32)) + (radius,)


@functools.lru_cache(maxsize=None)
def ref(name, order="ascending"):
    """The reference of a case, computed once and shared by the tests that need it."""
    import fpfh_radius_ref as FR
    xyz, nrm, radius = case(name)
    return FR.fpfh_radius(xyz, nrm, radius, order=order)
