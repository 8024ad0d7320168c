"""The numpy reference of FPFHEstimation (tests/fpfh_ref.py) against hand-computed values, its own invariants and a recorded result.
No GPU: what is checked here is the yardstick of tests/test_fpfh_gpu.py, not the engine."""
import functools
import itertools
import os

import numpy as np
import pytest

import fpfh_cases as K
import fpfh_ref as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fpfh_small.npz")


@functools.lru_cache(maxsize=None)
def _ref(name, k):
    return F.fpfh(K.cloud(name), K.ref_normals(name), k)


def test_hand_computed_pair():
    """Two points one unit apart along x, normals (0, 0, 1) and (0.6, 0, 0.8).  From record 0: a1 = 0, a2 = 0.6, so the roles
    swap: n1 = (0.6, 0, 0.8), dp = (-1, 0, 0), f3 = -0.6 -> 11 * 0.2 = 2.2, bin 2; v = dp x n1 = (0, 0.8, 0) -> (0, 1, 0),
    f2 = v . (0, 0, 1) = 0 -> 5.5, bin 5; w = n1 x v = (-0.8, 0, 0.6), f1 = atan2(0.6, 0.8) = 0.6435 -> 11 * 0.6024 = 6.63, bin 6.
    From record 1: a1 = -0.6, a2 = 0, no swap, the same n1, n2 and dp, so the same bins.  k = 2: hist_incr = 100, each block holds
    one 100; the FPFH of each record is the other's SPFH times 1 / d2 = 1, normalised: the same row."""
    xyz = np.float32([[0, 0, 0], [1, 0, 0]])
    nrm = np.float32([[0, 0, 1], [0.6, 0, 0.8]])
    r = F.fpfh(xyz, nrm, 2)
    want = np.zeros(33, np.float32)
    want[[6, 11 + 5, 22 + 2]] = 100.0
    assert r.idx.tolist() == [[0, 1], [1, 0]] and r.d2.tolist() == [[0.0, 1.0], [0.0, 1.0]]
    assert (r.spfh == want).all() and (r.fpfh == want).all()
    assert r.valid.tolist() == [[False, True], [False, True]]
    np.testing.assert_allclose(r.scaled[0, 1], [11 * (np.arctan2(0.6, 0.8) + np.pi) / (2 * np.pi), 5.5, 2.2], atol=1e-6)
    np.testing.assert_allclose(r.margin[:, 1], 0.2, atol=1e-6)               # f3 = 2.2 is the closest to an edge
    assert not r.fragile.any() and not r.nan_rows.any()


def test_skipped_pairs_and_table():
    """Coincident points, a dp along the source normal and a NaN normal are skipped; hist_incr keeps k - 1; the table is the
    sequential float sum."""
    xyz = np.float32([[0, 0, 0], [0, 0, 0], [0, 0, 1], [1, 0, 0]])
    nrm = np.float32([[0, 0, 1], [0, 0, 1], [0, 0, 1], [np.nan, 0, 0]])
    r = F.fpfh(xyz, nrm, 4)
    # record 0: itself, its copy (f4 = 0), record 2 (dp parallel to both normals: |v| = 0), record 3 (NaN normal): nothing counts
    assert r.counts[0].sum() == 0 and (r.spfh[0] == 0).all()
    assert r.nan_rows.tolist() == [False, False, False, True] and np.isnan(r.fpfh[3]).all() and (r.spfh[3] == 0).all()
    assert (r.fpfh[:3] == 0).all()                                             # sums of zeros: no division by zero
    tab = F.count_table(4)
    third = np.float32(100.0) / np.float32(3.0)
    assert tab[0] == 0 and tab[1] == third and tab[3] == np.float32(np.float32(third + third) + third)


@pytest.mark.parametrize("name,k", [("uniform", 10), ("sphere", 16), ("corner", 10), ("plane", 9), ("lattice", 10), ("copies", 10)])
def test_blocks_sum_to_100_or_are_zero(name, k):
    r = _ref(name, k)
    assert not r.nan_rows.any()
    assert F.blocks_ok(r.fpfh).all()
    # every counted pair is counted once per feature; SPFH blocks hold (pairs) * hist_incr
    pairs = r.valid.sum(axis=1)
    assert (r.counts.reshape(-1, 3, 11).sum(axis=2) == pairs[:, None]).all()
    full = pairs == k - 1
    assert np.abs(r.spfh[full].reshape(-1, 3, 11).astype(np.float64).sum(axis=2) - 100.0).max() <= 1e-3
    if name == "plane":                                                        # every feature at mid-bin: one bin per block
        assert (r.counts[:, [5, 16, 27]].sum(axis=1) == 3 * pairs).all()
    if name == "copies":                                                       # 13 records in one place, k = 10: nothing at a positive distance
        pile = [7] + list(range(1500, 1512))
        assert (r.d2[pile] == 0).all() and (r.fpfh[pile] == 0).all() and (r.spfh[pile] == 0).all()
        mixed = [100, 1512, 1513, 1514]                                        # 4 in one place: 6 neighbours at a positive distance
        assert ((r.d2[mixed] == 0).sum(axis=1) == 4).all() and (r.valid[mixed].sum(axis=1) == 6).all()
        assert F.blocks_ok(r.fpfh[mixed]).all() and (r.fpfh[mixed] != 0).any(axis=1).all()


def _rotations():
    """The 24 proper rotations of the cube: signed axis permutations of determinant +1, exact in float."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for row, (col, s) in enumerate(zip(perm, signs)):
                R[row, col] = s
            if np.linalg.det(R) > 0:
                out.append(R.astype(np.float32))
    assert len(out) == 24
    return out


def test_counts_survive_axis_permutations_and_sign_flips():
    """A signed axis permutation moves no bit of a coordinate, so the features change by the order of three-term float64 sums at
    most (about 1e-16): the counts of every record that is not fragile in either pose are identical.  The neighbourhoods are
    those of the first pose: the order of the three squares in a float32 d2 is not what is under test."""
    xyz, nrm = K.cloud("corner")[::5], K.ref_normals("corner")[::5]
    base = F.fpfh(xyz, nrm, 10)
    for R in _rotations():
        moved = F.fpfh(xyz @ R.T, nrm @ R.T, 10, knn_result=(base.idx, base.d2))
        ok = ~(base.fragile | moved.fragile)
        assert ok.mean() > 0.99
        assert (moved.counts[ok] == base.counts[ok]).all()


def test_recorded_result():
    """tests/golden/fpfh_small.npz: 64 points of the corner and their normals, k = 8, as this reference computed them when it was
    written.  Counts and FPFH rows of the records that were not fragile then are the same now."""
    g = np.load(GOLDEN)
    r = F.fpfh(g["xyz"], g["normals"], int(g["k"]))
    ok = ~g["fragile_nb"]
    assert ok.sum() >= 60 and (r.idx == g["idx"]).all()
    assert (r.counts[ok] == g["counts"][ok]).all()
    assert r.fpfh[ok].tobytes() == g["fpfh"][ok].tobytes()
    assert (r.fragile_nb == g["fragile_nb"]).all()


@functools.lru_cache(maxsize=None)
def _hand_made(name):
    xyz, nrm = K.HAND_MADE[name]()
    return F.fpfh(xyz, nrm, 10)


def _clamped(r, t):
    """The counted pairs whose scaled feature t lies outside [0, 11): the clamp moves them into bin 0 or bin 10."""
    s = r.scaled[..., t]
    return r.valid & ((s < 0.0) | (s >= float(F.BINS)))


@pytest.mark.parametrize("name", sorted(K.HAND_MADE))
def test_hand_made_normals(name):
    """The cases with normals that are not unit vectors, on the reference alone: the branches each one is there for are taken, the
    share of records the GPU test lets off stays under the cap (1 %; 4 % where two normals are zero and theta = +-pi hangs on the
    sign of a zero), and no row holds a NaN."""
    r = _hand_made(name)
    n = len(r.idx)
    own = np.arange(n)[:, None]
    pairs, skipped = int(r.valid.sum()), int((~r.valid & (r.idx != own)).sum())
    f2, f3 = int(_clamped(r, 1).sum()), int(_clamped(r, 2).sum())
    share = r.fragile_nb.mean()
    print("%s: %d records, %d pairs counted, %d skipped, clamped in f2 %d, in f3 %d, fragile %d, fragile or fragile neighbour %d (%.2f %%)" %
          (name, n, pairs, skipped, f2, f3, int(r.fragile.sum()), int(r.fragile_nb.sum()), 100 * share))
    assert n <= 2000 and share <= K.FRAGILE_CAP[name]
    assert not r.nan_rows.any() and np.isfinite(r.fpfh).all() and F.blocks_ok(r.fpfh).all()
    assert (r.counts.reshape(n, 3, 11).sum(axis=2) == r.valid.sum(axis=1)[:, None]).all()
    if name.startswith("non_unit"):
        assert f3 >= pairs / 4 and f2 > 0 and not r.fragile_nb.any() and skipped == 0
        assert r.counts[:, 22].sum() > 1000 and r.counts[:, 32].sum() > 1000 and r.counts[:, 11].sum() > 100 and r.counts[:, 21].sum() > 100   # both clamps
    if name == "parallel":
        assert skipped > 3000 and not r.fragile.any() and f2 == 0 and f3 == 0
        m = r.margin[r.valid]
        assert m.min() > 0.3                                                   # mid-bin (5.5) or well inside one (1.61, 9.39; 2.32 at the rim)
    if name == "zero_normals":
        a, b = K.ZEROED
        assert r.idx[a, 1] == b and r.idx[b, 1] == a                           # mutual nearest neighbours: v = 0 both ways
        assert not r.valid[a, 1] and not r.valid[b, 1] and skipped == 2
        assert r.fragile[a] and r.fragile[b] and 0 < r.fragile.sum() < 20      # theta = +-pi on the sign of a zero
        s = r.scaled[[a, b]][r.valid[[a, b]]]
        assert np.isin(s[:, 0], [0.0, 5.5, 11.0]).all() and (s[:, 1] == 5.5).all()   # atan2(+-0, +-0) is 0 or +-pi; f2 = v . 0 = 0


def test_every_k_lets_no_record_off():
    """uniform(200, 3) at every k from 2 to 64: no record is fragile at any k, so the GPU sweep compares every row."""
    xyz, nrm = K.every_k()
    assert len(xyz) == 200 and K.EVERY_K == tuple(range(2, 65))
    for k in K.EVERY_K:
        r = F.fpfh(xyz, nrm, k)
        assert not r.fragile_nb.any() and not r.nan_rows.any() and F.blocks_ok(r.fpfh).all(), k
        assert (r.valid.sum(axis=1) == k - 1).all()


@pytest.mark.parametrize("name,k", [("uniform", 10), ("sphere", 16), ("corner", 10), ("plane", 9), ("lattice", 10)])
def test_fragile_share(name, k):
    """The cap: at most 1 % of the records are fragile or have a fragile neighbour, on the reference alone.  The 12^3 lattice is
    exempt (its cube neighbourhoods have no defined normal, so features sit on edges by construction), not from being computed."""
    r = _ref(name, k)
    share = r.fragile_nb.mean()
    m = r.margin[np.isfinite(r.margin)]
    print("%s k=%d: fragile %.2f %%, fragile or fragile neighbour %.2f %%, smallest margin %.3g bins" %
          (name, k, 100 * r.fragile.mean(), 100 * share, m.min() if len(m) else np.inf))
    if name != "lattice":
        assert share <= 0.01
