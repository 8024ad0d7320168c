"""CPU: the C oracle's edge extractor (oracle/edge_oracle.c) against the staged numpy reference (tests/edges_ref.py) on every image
of tests/edges_cases.py, index for index -- and, on the reference's stages, the property each image is there for: an image that
does not reach what it is meant to reach fails here, before the GPU tests (tests/test_edges_gpu.py) rely on it."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import edges_cases as E
import edges_ref as R

T = E.TILE
JOINS = {"W": (0, -1), "NW": (-1, -1), "N": (-1, 0), "NE": (-1, 1)}


@pytest.mark.parametrize("group", E.GROUPS)
def test_oracle_equals_reference(orc, group):
    for name in E.names(group):
        pts, w, h = E.build(name)
        np.testing.assert_array_equal(orc.edge_features(pts, w, h), E.indices(name), err_msg=name)


def test_oracle_equals_reference_on_every_step_height(orc):
    for o in E.THRESHOLD_ORIENTATIONS:
        for delta in range(256):
            pts, w, h = E.threshold_step(o, delta)
            idx = orc.edge_features(pts, w, h)
            np.testing.assert_array_equal(idx, R.edge_indices(pts, w, h), err_msg="%s %d" % (o, delta))
            assert len(idx) == E.threshold_sweep(o)[delta][1]


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wh", sorted(E.SHAPES))
def test_shapes_reach_the_borders_and_the_last_tile(wh):
    w, h = wh
    s = E.stages("shape_%dx%d" % (w, h))
    assert s.keep[1].any() and s.keep[h - 2].any() and s.keep[:, 1].any() and s.keep[:, w - 2].any()
    assert not s.keep[0].any() and not s.keep[h - 1].any() and not s.keep[:, 0].any() and not s.keep[:, w - 1].any()
    # the last, partial tile: one pixel wide it holds border pixels only, which the suppression never keeps -- then column
    # w - 2 above is the last column of a full tile, whose halo is that one pixel, clamped
    if w % T > 1:
        assert s.keep[:, w - w % T:].any()
    if h % T > 1:
        assert s.keep[h - h % T:].any()
    rgba = E.build("shape_%dx%d" % (w, h))[0]["rgba"].astype(np.int64)
    sums = (rgba & 255) + ((rgba >> 8) & 255) + ((rgba >> 16) & 255)
    assert (sums % 3 != 0).any() and (len(np.unique(sums % 3)) == 3 or w * h < 16)     # channel sums that are no multiples of 3


def test_step_3x3():
    np.testing.assert_array_equal(E.indices("shape_step_3x3"), [4])


# ---- seams -----------------------------------------------------------------------------------------------------------------------
def joins(s):
    """every join between two edge points (i, j) and its W / NW / N / NE neighbour: kind -> (i, j) arrays of the first"""
    out = {}
    for kind, (di, dj) in JOINS.items():
        ii, jj = np.nonzero(s.keep)
        ok = (ii + di >= 0) & (jj + dj >= 0) & (jj + dj < s.w)
        ii, jj = ii[ok], jj[ok]
        ok = s.keep[ii + di, jj + dj]
        out[kind] = (ii[ok], jj[ok])
    return out


def crosses_tiles(kind, i, j):
    di, dj = JOINS[kind]
    return ((i + di) // T != i // T) | ((j + dj) // T != j // T)


def indices_without(s, dropped):
    """the edge points if the joins for which dropped(kind, i, j) holds were never made (kept pixels, both thresholds as in the
    reference)"""
    kept = s.mx != 0
    n = s.w * s.h
    rows, cols = [], []
    for kind, (di, dj) in JOINS.items():
        ii, jj = np.nonzero(kept)
        ok = (ii + di >= 0) & (jj + dj >= 0) & (jj + dj < s.w)
        ii, jj = ii[ok], jj[ok]
        ok = kept[ii + di, jj + dj] & ~dropped(kind, ii, jj)
        rows.append(ii[ok] * s.w + jj[ok])
        cols.append((ii[ok] + di) * s.w + jj[ok] + dj)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    _, lab = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n)), directed=False)
    strong = np.zeros(n, bool)
    strong[lab[(kept & ~(s.mx < R.T_HIGH)).reshape(-1)]] = True
    return np.flatnonzero(strong[lab] & kept.reshape(-1))


@pytest.fixture(scope="module")
def seam_stages():
    return {name: E.stages(name) for name in E.names("seams")}


def test_indices_without_nothing_dropped_is_the_reference(seam_stages):
    for name in list(seam_stages)[::7]:
        s = seam_stages[name]
        np.testing.assert_array_equal(indices_without(s, lambda kind, i, j: np.zeros(len(i), bool)), s.indices)


def test_seams_cross_tiles_through_every_join(seam_stages):
    seen = {k: 0 for k in JOINS}
    corners = {"NW into the diagonal tile": 0, "NE into the diagonal tile": 0, "NE from a last column below the first row": 0}
    for s in seam_stages.values():
        for kind, (i, j) in joins(s).items():
            x = crosses_tiles(kind, i, j)
            seen[kind] += int(x.sum())
            if kind == "NW":
                corners["NW into the diagonal tile"] += int((x & (i % T == 0) & (j % T == 0)).sum())
            if kind == "NE":
                corners["NE into the diagonal tile"] += int((x & (i % T == 0) & (j % T == T - 1)).sum())
                corners["NE from a last column below the first row"] += int((x & (i % T != 0) & (j % T == T - 1)).sum())
    assert all(v > 0 for v in seen.values()), seen
    assert all(v > 0 for v in corners.values()), corners


# the joins across tile edges, by the branch of k_edge_cc_borders that makes them: without any one of these classes some seam
# image must lose edge points, or no comparison of indices can tell whether the branch is there
BRANCHES = {
    "W from a first column": lambda kind, i, j: (kind == "W") & (j % T == 0),
    "N from a first row": lambda kind, i, j: (kind == "N") & (i % T == 0),
    "NW from a first row, not the corner": lambda kind, i, j: (kind == "NW") & (i % T == 0) & (j % T != 0),
    "NW from a first column, not the corner": lambda kind, i, j: (kind == "NW") & (i % T != 0) & (j % T == 0),
    "NW from the corner": lambda kind, i, j: (kind == "NW") & (i % T == 0) & (j % T == 0),
    "NE from a first row, not the corner": lambda kind, i, j: (kind == "NE") & (i % T == 0) & (j % T != T - 1),
    "NE from a last column below the first row": lambda kind, i, j: (kind == "NE") & (i % T != 0) & (j % T == T - 1),
    "NE from the corner": lambda kind, i, j: (kind == "NE") & (i % T == 0) & (j % T == T - 1),
}


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_some_seam_needs_each_branch_of_the_border_joins(seam_stages, branch):
    needed = [name for name, s in seam_stages.items() if len(indices_without(s, BRANCHES[branch])) != len(s.indices)]
    assert needed, branch


def test_a_component_hangs_on_strong_pixels_tiles_away_from_its_root(seam_stages):
    found = []
    for name, s in seam_stages.items():
        for root in np.unique(s.root[s.keep]):
            i, j = np.nonzero(s.root == root)
            tiles = set(zip(i // T, j // T))
            strong = ~(s.mx[i, j] < R.T_HIGH)
            root_tile = (root // s.w // T, root % s.w // T)
            if len(tiles) >= 6 and strong.any() and root_tile not in set(zip(i[strong] // T, j[strong] // T)):
                found.append(name)
    assert found
    # ... in every orientation, and the strong end in the first tiles of the path as well as in the last
    assert {n.split("_")[1] for n in found} == set(E.SEAM_ORIENTATIONS)
    for o in E.SEAM_ORIENTATIONS:
        for end in ("first", "last"):
            spans = [len(set(zip(*(np.nonzero(s.keep)[0] // T, np.nonzero(s.keep)[1] // T)))) for n, s in seam_stages.items()
                     if n.startswith("seam_%s_%s_" % (o, end))]
            assert max(spans) >= 3, (o, end)


def test_the_weak_part_of_a_seam_alone_has_no_edge_point(seam_stages):
    for o in E.SEAM_ORIENTATIONS:
        for last in (0, 1):
            for ox in E.SEAM_OFFSETS:
                for oy in E.SEAM_OFFSETS:
                    pts, w, h = E.seam(o, last, ox, oy, weak_only=True)
                    s = R.canny(pts["rgba"], w, h)
                    assert (s.mx != 0).sum() > 30 and len(s.indices) == 0, (o, last, ox, oy)
                    whole = seam_stages["seam_%s_%s_%d_%d" % (o, "last" if last else "first", ox, oy)]
                    # the whole image keeps weak pixels of that part: they hang on the strong end
                    assert (whole.keep & (s.mx != 0)).sum() > 30, (o, last, ox, oy)


# ---- thresholds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orientation", E.THRESHOLD_ORIENTATIONS)
def test_step_heights_lie_on_both_sides_of_both_thresholds(orientation):
    sweep = E.threshold_sweep(orientation)
    mags, counts = [m for m, _ in sweep], [c for _, c in sweep]
    first = min(d for d in range(256) if counts[d])
    assert 0 < first < 255 and not any(counts[:first]) and all(counts[first:])
    j = E.just(orientation)
    assert mags[j["below_weak"]] < 40.0 <= mags[j["weak"]] and mags[j["below_strong"]] < 100.0 <= mags[j["strong"]]
    assert first == j["strong"]
    for d in range(1, 256):
        assert mags[d] > mags[d - 1]


def test_two_level_images_hold_a_just_weak_step_kept_and_dropped():
    kept_weak = dropped_weak = 0
    for name in E.names("two_level"):
        s = E.stages(name)
        weak = (s.mx != 0) & (s.mx < R.T_HIGH)
        kept_weak += int((weak & s.keep).sum())
        dropped_weak += int((weak & ~s.keep).sum())
    assert kept_weak > 0 and dropped_weak > 0


def test_magnitudes_lie_exactly_on_both_thresholds():
    """!(mx < 100) against mx > 100 and !(m < 40) against m > 40 differ only at equality: there are components whose only pixels
    not below 100 are 100.0f exactly (with > their points are gone), and edge points with mx == 40.0f exactly"""
    only_exact, at_low, both = [], [], []
    for name in E.names("exact"):
        s = E.stages(name)
        strong = s.keep & ~(s.mx < R.T_HIGH)
        hangs_on_exact = [r for r in np.unique(s.root[s.keep]) if (s.mx[strong & (s.root == r)] == R.T_HIGH).all()]
        low = int((s.keep & (s.mx == R.T_LOW)).sum())
        if hangs_on_exact:
            only_exact.append(name)
        if low:
            at_low.append(name)
        if hangs_on_exact and low:
            both.append(name)
    assert "exact_step" in only_exact and "exact_step_T" in only_exact and len(E.indices("exact_step")) == 12
    assert len(only_exact) >= 4 and len(at_low) >= 4 and both, (only_exact, at_low, both)


# ---- suppression ties ------------------------------------------------------------------------------------------------------------
def along_gradient(s):
    """the magnitudes of the two neighbours along the direction class, (h - 2, w - 2) each, for the interior pixels"""
    a, b = np.zeros((s.h - 2, s.w - 2), np.float32), np.zeros((s.h - 2, s.w - 2), np.float32)
    d = s.dir[1:-1, 1:-1]
    for c, (di, dj) in R.NEIGHBOUR.items():
        a = np.where(d == c, s.mag[1 + di:s.h - 1 + di, 1 + dj:s.w - 1 + dj], a)
        b = np.where(d == c, s.mag[1 - di:s.h - 1 - di, 1 - dj:s.w - 1 - dj], b)
    return a, b


def test_suppression_meets_equal_and_barely_larger_neighbours():
    equal = by_an_ulp = 0
    for name in E.names("ties", "directions", "exact"):
        s = E.stages(name)
        a, b = along_gradient(s)
        m, kept = s.mag[1:-1, 1:-1], s.keep[1:-1, 1:-1]          # (edge points: with > in the suppression the indices change)
        equal += int((kept & ((a == m) | (b == m))).sum())
        hi = np.maximum(a, b)
        # dropped although not below the low threshold and of a valid class, by a neighbour larger by exactly one ulp
        close = hi == np.nextafter(m, np.float32(np.inf))
        by_an_ulp += int((~kept & ~(m < R.T_LOW) & (s.dir[1:-1, 1:-1] != 255) & close).sum())
    assert equal > 0 and by_an_ulp > 0, (equal, by_an_ulp)


# ---- directions ------------------------------------------------------------------------------------------------------------------
def test_directions_reach_every_class_and_every_boundary():
    classes, near = set(), {b: 0 for b in R.CLASS_BOUNDARIES}
    gx0 = gy0 = diag = 0
    for name in E.names("directions", "shapes"):
        s = E.stages(name)
        kept = s.mx != 0
        classes |= set(np.unique(s.dir[kept]).tolist())
        for b in near:
            near[b] += int((kept & (np.abs(s.angle - np.float32(b)) < 0.5)).sum())
        live = kept
        gx0 += int((live & (s.gx == 0)).sum())
        gy0 += int((live & (s.gy == 0)).sum())
        diag += int((live & (np.abs(s.gx) == np.abs(s.gy))).sum())
    assert classes == {0, 1, 2, 3}
    assert all(v > 0 for v in near.values()), near
    assert gx0 > 0 and gy0 > 0 and diag > 0, (gx0, gy0, diag)


def test_direction_boundaries_are_met_from_both_sides():
    below, above = {b: 0 for b in R.CLASS_BOUNDARIES}, {b: 0 for b in R.CLASS_BOUNDARIES}
    for name in E.names("directions"):
        s = E.stages(name)
        big = ~(s.mag < R.T_LOW)
        for b in below:
            d = s.angle - np.float32(b)
            below[b] += int((big & (d < 0) & (d > -0.5)).sum())
            above[b] += int((big & (d >= 0) & (d < 0.5)).sum())
    assert all(below.values()) and all(above.values()), (below, above)


# ---- records and compaction ------------------------------------------------------------------------------------------------------
def test_records_cases():
    base = E.indices("shape_97x70")
    for name in ("records_stride20", "records_stride48", "records_alpha", "records_non_finite", "records_non_finite_stride20"):
        np.testing.assert_array_equal(E.indices(name), base, err_msg=name)
    assert E.build("records_stride20")[0].dtype.itemsize == 20 and E.build("records_stride48")[0].dtype.itemsize == 48
    assert (E.build("records_stride48")[0]["extra"] == 0xdeadbeef).all()
    nf = E.build("records_non_finite")[0]
    for f in ("x", "y", "z", "w"):
        assert np.isnan(nf[f]).any() and np.isinf(nf[f]).any() and ((nf[f] != 0) & (np.abs(nf[f]) < 1e-38)).any()
    assert len(np.unique(E.build("records_alpha")[0]["rgba"] >> 24)) == 256
    assert len(E.indices("records_only_r")) > 0
    np.testing.assert_array_equal(E.indices("records_only_r"), E.indices("records_only_b"))
    assert len(E.indices("records_only_alpha")) == 0 and len(E.indices("records_only_x")) == 0
    a, x = E.build("records_only_alpha")[0], E.build("records_only_x")[0]
    assert len(np.unique(a["rgba"] >> 24)) > 100 and len(np.unique(x["x"])) > 100


def test_compaction_cases_fill_the_blocks_they_name():
    blocks = lambda name: sorted(set((E.indices(name) // E.BLOCK).tolist()))
    assert E.COMPACT_W * E.COMPACT_H == 3 * E.BLOCK + 322
    assert blocks("compaction_first") == [0]
    assert blocks("compaction_last") == [3]
    assert blocks("compaction_first_and_last") == [0, 3]
    assert blocks("compaction_dense") == [0, 1, 2, 3]
    assert blocks("compaction_flat") == []
