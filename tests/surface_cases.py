"""Inputs of the search-surface tests (tests/test_surface_cpu.py, tests/test_surface_gpu.py): the surfaces are the clouds of
fpfh_radius_cases with their normals and radius; the queries of a case are a seeded pick of one surface record in `pick`, each
moved by up to +-0.3 radius along every axis, then five exact surface records, one query at (50, 50, 50) and one at (-3, 0.2, 0.1)
-- both more than a radius from every surface here: m = 0.  In `holes` the surface has non-finite records (a picked one is a
non-finite query) and non-finite normals.  Everything float32, made once.

The caps are CONDITIONS on the inputs, decided on the reference alone (tests/test_surface_cpu.py checks every case, the GPU test
again): those of fpfh_radius_cases -- at most 5 % of the queries with a fragile surface neighbour, at most 1 value in 10 000 moved
when the float64 sums run in descending instead of ascending order -- and a needed share (surface records that are a neighbour of
a query) below 80 % in the SUBSET cases: a call that needs every row would not show that the others are left out.
"""
import functools

import numpy as np

import fpfh_radius_cases as C

FRAGILE_NB_CAP, DIFFER_CAP, NEEDED_CAP = C.FRAGILE_NB_CAP, C.DIFFER_CAP, 0.8
FAR = np.float32([[50.0, 50.0, 50.0], [-3.0, 0.2, 0.1]])
JITTER = 0.3

# (surface case of fpfh_radius_cases, pick one record in)
CASES = [("corner_0.05", 40), ("corner_0.05", 8), ("corner_0.12", 40), ("sphere_0.2", 40), ("uniform_0.12", 20), ("holes", 20)]
IDS = ["%s-1/%d" % c for c in CASES]
# the cases whose queries reach a part of the surface only: the needed share is capped there (sphere_0.2: a ball of 0.2 around 50
# queries covers nine tenths of a shell of radius 0.5 -- it is here for its neighbourhoods of a hundred and its fragile rows)
SUBSET = [c for c in CASES if c[0] != "sphere_0.2"]


@functools.lru_cache(maxsize=None)
def queries(name, pick):
    """(nq, 3) float32: the jittered pick, five exact surface records, the two far queries."""
    xyz, _, radius = C.case(name)
    rng = np.random.default_rng(1000 + pick)
    chosen = np.sort(rng.choice(len(xyz), len(xyz) // pick, replace=False))
    moved = xyz[chosen] + (rng.uniform(-JITTER, JITTER, (len(chosen), 3)) * radius).astype(np.float32)
    fin = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    exact = xyz[fin[np.linspace(0, len(fin) - 1, 5).astype(np.int64)]]
    q = np.ascontiguousarray(np.concatenate([moved, exact, FAR]), np.float32)
    q.setflags(write=False)
    return q


def case(name, pick):
    """(queries, surface, surface normals, radius)"""
    xyz, nrm, radius = C.case(name)
    return queries(name, pick), xyz, nrm, radius


@functools.lru_cache(maxsize=None)
def ref_search(name, pick):
    import surface_ref as SR
    q, s, _, radius = case(name, pick)
    return SR.search(q, s, radius)


@functools.lru_cache(maxsize=None)
def ref(name, pick, order="ascending"):
    """surface_ref.fpfh of a case, computed once and shared by the tests that need it; the surface's own reference is
    fpfh_radius_cases.ref's."""
    import surface_ref as SR
    q, s, nrm, radius = case(name, pick)
    return SR.fpfh(q, s, nrm, radius, order=order, nb=ref_search(name, pick), surface_ref=C.ref(name))


@functools.lru_cache(maxsize=None)
def ref_normals(name, pick, viewpoint=(0.0, 0.0, 0.0)):
    import surface_ref as SR
    q, s, _, radius = case(name, pick)
    return SR.normals(q, s, radius, viewpoint, nb=ref_search(name, pick))
