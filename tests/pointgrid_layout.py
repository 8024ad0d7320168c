"""grid_layout of csrc/pointgrid.hpp restated in plain Python, and the float32 arithmetic that places a point in a cell and bounds
the distance to a cell (cell_pos, axis_cell, axis_gap, grid_lb2, l2_simple of csrc/records.hpp and csrc/pointgrid.hpp).

Only doubles, floor and sqrt enter grid_layout, and Python's float is the same IEEE double: layout() agrees with the C++ bit for
bit (tests/test_pointgrid_layout_cpu.py holds it against tests/cpp/grid_layout.cpp).  The float32 helpers round every step, as
the device code does with its __f*_rn intrinsics and -ffp-contract=off.

The five rules that can fix the cell, as layout() names them in `branch`:
  "bisection"   about kCellsPerPoint cells per finite point (the geometric bisection between the floor and two cells per axis);
  "emax/4000"   never more than 4 000 cells (+ 2) along an axis;
  "big*1e-5"    never so small that the rounding of a coordinate is a sizeable part of it;
  "emax==0"     every finite point in one place: max(big * 1e-5, 1);
  "min_cell"    the radius of a radius search (`capped`: by two cells per axis, min_cell > 2 * max(emax, floor)).
("1e-30": the guard against a zero cell, reached by denormal boxes only.)
"""
import collections
import math

import numpy as np

# kCellsPerPoint, kMinCells, kMaxCells, kBlocks
POLICIES = {"knn": (64.0, 4096.0, 33554432.0, False), "radius": (64.0, 4096.0, 33554432.0, False), "fit": (4.0, 64.0, 16777216.0, True)}
CELL_MARGIN = np.float32(0.03)      # kCellMargin
LB_FACTOR = np.float32(0.999996)    # grid_lb2's relative factor
LB_DENORMAL_SLACK = np.float32(2.0 ** -147)   # ... and what it takes off for a d2 in the float32 denormals
GRID_MAX_AXIS = 4096                # kGridMaxAxis

Layout = collections.namedtuple("Layout", "cell inv_cell dims branch origin capped")


def layout(mn, mx, nfin, policy, min_cell=0.0):
    """grid_layout<Policy>(mn, mx, nfin, gx, min_cell): (cell f32, inv_cell f32, dims, branch, origin f32[3], capped)."""
    per_point, min_cells, max_cells, blocks = POLICIES[policy]
    mn, mx = np.asarray(mn, np.float32), np.asarray(mx, np.float32)
    e = [float(mx[k]) - float(mn[k]) for k in range(3)]
    emax = max(0.0, *e)
    big = max(0.0, *[max(abs(float(mn[k])), abs(float(mx[k]))) for k in range(3)])
    target = min(max(per_point * int(nfin), min_cells), max_cells)

    def cells_along(k, c):
        d = int(math.floor(e[k] / c)) + 2
        return (d + 3) & ~3 if blocks else d

    def cells_for(c):
        return float(cells_along(0, c)) * float(cells_along(1, c)) * float(cells_along(2, c))

    terms = {"emax/4000": emax / 4000.0, "big*1e-5": big * 1e-5, "1e-30": 1e-30}
    lo = max(terms.values())
    branch = [name for name, v in terms.items() if v == lo][0]
    if emax == 0:
        lo = max(big * 1e-5, 1.0)
        branch = "emax==0"
    cap = max(emax, lo) * 2.0
    clamp = min(float(min_cell), cap)
    capped = False
    if clamp > lo:
        lo, branch, capped = clamp, "min_cell", float(min_cell) > cap
    cell = lo
    if cells_for(lo) > target:
        hi = max(emax, lo) * 2.0
        for _ in range(100):
            mid = math.sqrt(lo * hi)
            if cells_for(mid) > target:
                lo = mid
            else:
                hi = mid
        cell, branch, capped = hi, "bisection", False
    cell32 = np.float32(cell)
    inv32 = np.float32(1.0 / float(cell32))
    dims = tuple(cells_along(k, float(cell32)) for k in range(3))
    return Layout(cell32, inv32, dims, branch, mn.copy(), capped)


def box_of(xyz):
    """(min, max, number) of the finite records: what k_grid_box hands to grid_layout."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    fin = xyz[np.isfinite(xyz).all(axis=1)]
    return fin.min(axis=0), fin.max(axis=0), len(fin)


def layout_of(xyz, policy, min_cell=0.0):
    mn, mx, nfin = box_of(xyz)
    return layout(mn, mx, nfin, policy, min_cell)


def cell_pos(xyz, lay):
    """(p - origin) * inv_cell, both steps rounded to float32."""
    xyz = np.asarray(xyz, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return ((xyz - lay.origin).astype(np.float32) * lay.inv_cell).astype(np.float32)


POS_MAX = np.float32(1e18)          # kPosMax: beyond it a position says nothing the bounds can use


def bound_pos(u):
    """bound_pos: the position the bounds measure from -- NaN where (p - origin) has overflowed or lies beyond kPosMax cells."""
    u = np.asarray(u, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(u) <= POS_MAX, u, np.float32(np.nan)).astype(np.float32)


def cells_of(xyz, lay):
    """axis_cell along every axis: floor(cell_pos), clamped into the grid (fmaxf, then fminf: a NaN lands in cell 0, an overflowed
    position in the last cell).  int32, the shape of xyz."""
    u = np.floor(cell_pos(xyz, lay))
    top = np.asarray(lay.dims, np.float32) - np.float32(1)
    return np.fmin(np.fmax(u, np.float32(0)), top).astype(np.int32)


def axis_gap(u, lo, hi):
    """float32: fmaxf(fmaxf(lo - u, u - (hi + 1)) - kCellMargin, 0): 0 for a NaN position."""
    u = np.asarray(u, np.float32)
    with np.errstate(invalid="ignore"):
        a = (np.asarray(lo).astype(np.float32) - u).astype(np.float32)
        b = (u - (np.asarray(hi) + 1).astype(np.float32)).astype(np.float32)
        return np.fmax((np.fmax(a, b) - CELL_MARGIN).astype(np.float32), np.float32(0))


def grid_lb2(gx, gy, gz, cell):
    """float32: (((gx * gx + gy * gy + gz * gz) * 0.999996) * cell) * cell - 2^-147, left to right, every step rounded."""
    gx, gy, gz = (np.asarray(g, np.float32) for g in (gx, gy, gz))
    cell = np.float32(cell)
    with np.errstate(over="ignore", under="ignore"):
        s = ((gx * gx).astype(np.float32) + (gy * gy).astype(np.float32)).astype(np.float32)
        s = (s + (gz * gz).astype(np.float32)).astype(np.float32)
        s = (s * LB_FACTOR).astype(np.float32)
        s = (s * cell).astype(np.float32)
        s = (s * cell).astype(np.float32)
        return (s - LB_DENORMAL_SLACK).astype(np.float32)


def radius_reach(radius, lay):
    """radius_query: how far, in cells, a ball reaches along an axis -- float32(radius / cell * 1.00001 + 2 * kCellMargin)."""
    with np.errstate(over="ignore"):
        return np.float32(float(radius) / float(lay.cell) * 1.00001 + 2.0 * float(CELL_MARGIN))


def radius_axis_cells(u, reach, d):
    """radius_axis_cells: the cells lo .. hi along one axis that a ball around in-grid position u can touch (float32, clamped; a NaN
    position: the whole axis)."""
    u = np.asarray(u, np.float32)
    top = np.float32(d - 1)
    with np.errstate(invalid="ignore"):
        lo = np.fmin(np.fmax(np.floor((u - reach).astype(np.float32)), np.float32(0)), top).astype(np.int32)
        hi = np.fmax(np.fmin(np.floor((u + reach).astype(np.float32)), top), np.float32(0)).astype(np.int32)
    return lo, hi
