"""What tests/trips_cases.py claims about its clouds, held on the CPU with tests/pointgrid_layout.py (the grid's layout restated)
and the numpy references alone: the finite counts are as named, the two piles of two_trips_piles stand on either side of the
65 536-th place of the cell order in the k-NN grid and in the radius grids, the normals check leaves out no more than the existing
5 % cap, and the two radii give a few and most records fewer than three neighbours.

Measured with this construction (seed 1): left out 0.9 % at k = 10 and at k = 64 (the 600 pile records: every neighbour in one
place); fewer than three neighbours: 9 records at r = 0.05, 47 560 at r = 0.02.
"""
import functools

import numpy as np
import pytest

import normals_ref as N
import radius_ref as R
import trips_cases as T


@functools.lru_cache(maxsize=None)
def _knn(name, k):
    return N.knn(T.xyz(name), k)


@pytest.mark.parametrize("name", T.NAMES)
def test_finite_counts_and_trips(name):
    xyz = T.xyz(name)
    fin = np.isfinite(xyz).all(axis=1)
    assert int(fin.sum()) == T.NFIN[name]
    first, last, lay = T.cell_order_positions(xyz)
    assert lay.branch == "bisection"
    if name.startswith("launch_edge_"):
        bad = xyz[~fin]
        assert len(bad) == T.N_HOLES and np.isnan(bad).all(axis=1).sum() == T.N_HOLES // 2 and np.isinf(bad[:, 1]).sum() == T.N_HOLES // 2
        holes = np.flatnonzero(~fin)                          # spread through the cloud, and record ids beyond 65 535 on both sides
        assert holes.min() < 1000 and holes.max() > len(xyz) - 1000 and len(xyz) > T.LAUNCH_CAP + 1000
        assert fin[T.LAUNCH_CAP:].sum() > 1000
    want = {"two_trips_piles": 2, "launch_edge_65535": 1, "launch_edge_65536": 1, "launch_edge_65537": 2, "four_trips": 4}[name]
    assert T.trips(T.NFIN[name]) == want
    if name == "four_trips":                                  # workgroup 0 alone makes the fourth trip
        assert T.NFIN[name] - 3 * T.LAUNCH_CAP == 1
    # the records a second trip answers: cell-order places from 65 536 on, among them record ids on both sides of 65 535
    later = np.flatnonzero(first >= T.LAUNCH_CAP)
    if want > 1:
        assert len(later) >= 1 and (name == "launch_edge_65537" or ((later < T.LAUNCH_CAP).any() and (later >= T.LAUNCH_CAP).any()))


def test_piles_stand_on_either_side_of_the_launch_cap():
    xyz = T.xyz("two_trips_piles")
    lo, hi = T.piles()
    assert len(xyz) == 66600 and len(lo) == len(hi) == T.PILE == 300 > 256
    assert (xyz[lo] == xyz[:T.N_UNIFORM].min(axis=0)).all() and (xyz[hi] == xyz[:T.N_UNIFORM].max(axis=0)).all()
    for policy, min_cell in (("knn", 0.0),) + tuple(("radius", r) for r in T.RADII["two_trips_piles"]):
        first, last, lay = T.cell_order_positions(xyz, policy, min_cell)
        print("%s %g: grid %d x %d x %d (%s), first pile at %d .. %d, second at %d .. %d" %
              (policy, min_cell, *lay.dims, lay.branch, first[lo].min(), last[lo].max(), first[hi].min(), last[hi].max()))
        assert first[lo].min() == 0                           # cell 0: the head of the cell order
        assert (last[lo] < T.LAUNCH_CAP).all()                # trip 1 ...
        assert (first[hi] >= T.LAUNCH_CAP).all()              # ... and trip 2
        assert last[hi].max() == len(xyz) - 1                 # the last occupied cell
        # the workgroups of the first pile answer ordinary queries in trip 2; the second pile's ran an ordinary query in trip 1
        pile = np.zeros(len(xyz), bool)
        pile[np.r_[lo, hi]] = True
        second = np.flatnonzero((first >= T.LAUNCH_CAP) & (last < T.LAUNCH_CAP + 256))
        assert len(second) and not pile[second].any()
        before = np.flatnonzero((last >= first[hi].min() - T.LAUNCH_CAP) & (last < T.LAUNCH_CAP))
        assert len(before) >= T.PILE and not pile[before].any()


@pytest.mark.parametrize("k", [10, 64])
def test_share_the_normals_check_leaves_out(k):
    """On the reference alone: gap < 1e-3 on at most 5 % of the finite records (tests/test_normals_gpu.py's cap)."""
    xyz = T.xyz("two_trips_piles")
    ref = N.normals(xyz, k, knn_result=_knn("two_trips_piles", k))
    out = ref.gap[ref.finite] < 1e-3
    lo, hi = T.piles()
    print("two_trips_piles k = %d: left out %.2f %% (%d records)" % (k, 100 * out.mean(), int(out.sum())))
    assert out.mean() <= 0.05
    assert out[np.r_[lo, hi]].all() and (ref.trace[np.r_[lo, hi]] == 0).all()   # the piles: every neighbour in one place
    assert 600 <= out.sum() <= 610                                              # 0.9 %: the 600 pile records (and their two originals)


def test_by_hand_the_pile_s_neighbours():
    """Every record of a pile (and the uniform record it copies) has the 64 lowest record indices of that place as its neighbours."""
    xyz = T.xyz("two_trips_piles")
    idx, d2 = _knn("two_trips_piles", 64)
    for pile, corner in zip(T.piles(), (xyz[:T.N_UNIFORM].min(axis=0), xyz[:T.N_UNIFORM].max(axis=0))):
        place = np.flatnonzero((xyz == corner).all(axis=1))
        assert len(place) >= T.PILE and (np.isin(pile, place)).all()
        assert (idx[place] == place[:64]).all() and (d2[place] == 0).all()


def test_fewer_than_three_neighbours():
    xyz = T.xyz("two_trips_piles")
    few = {r: int((R.counts(xyz, r) < 3).sum()) for r in T.RADII["two_trips_piles"]}
    print("two_trips_piles: records with fewer than three neighbours:", few)
    assert few[0.05] == 9                                     # a few ...
    assert few[0.02] == 47560 and few[0.02] > len(xyz) // 2   # ... and most
    for name in ("launch_edge_65537", "four_trips"):          # the other cases: some rows are NaN, most are not
        c = R.counts(T.xyz(name), T.RADII[name][0])
        fin = np.isfinite(T.xyz(name)).all(axis=1)
        assert 0 < (c[fin] < 3).sum() < fin.sum() // 100
