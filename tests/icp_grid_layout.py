"""icp_grid_plan of csrc/icp_grid_plan.hpp restated in plain Python -- the grid of the ICP correspondence search: cell, origin, dims,
max_ring and the kind of index -- and a cost model of the searches that run over it.  tests/test_icp_scale_cpu.py holds plan()
against tests/cpp/icp_grid_plan.cpp, which runs the header itself.

Only doubles, floor, ceil, sqrt and pow enter the rule, and Python's float is the same IEEE double; the steps the header does in
float32 (the cell, its inverse, host_cell_coord) are rounded to float32 here, one operation at a time.

The cost model: an upper bound on what ONE query can touch
--------------------------------------------------------
A "touch" is one trip of a loop of the far search (a brick probed or passed over, a row opened or passed over), one cell or
occupancy word of the near search, or one target point scored.  cost_bound(plan, limit, n_points) bounds it for a query ANYWHERE,
from the loops of csrc/icp_kernels.hpp (nn_far_global) and csrc/icp_dense.hpp (dense_far, dense_far_blocks), given only the
distance `limit` the search can never look beyond: the gate, or +inf for an unbounded one.  (The running limit of a query is
min(gate^2, best d2 so far), so the gate bounds it whatever the query finds, and +inf means: nothing does.)

  near       rings 0-1 are 27 cells in at most 8 bricks, or 27 cells and 3 occupancy words: NEAR = 36 touches, and the seed is one point.
  points     a far search opens every brick and every row at most once, and never a cell of rings 0-1 again: every target point is
             scored at most once: n_points + 1 touches.
  far, brick hash (nn_far_global)
             nothing when max_ring <= 1 or limit <= (1 - margin) * cell.  Else shells rb = 0 .. R of bricks around the query's own, with
               rb_max = min(rb_grid, (max_ring + 3) // 4 + 1),   rb_grid <= max(nb_k) - 1   (nb_k = (dims_k + 3) >> 2 bricks along axis k)
               R = min(rb_max, R_stop),  R_stop = the first rb with limit <= (4 rb - margin) * cell = ceil((limit / cell + margin) / 4)
             (+ 1 here, for the float32 rounding of both sides of that comparison).  Shell rb runs 2 rb + 1 trips of the dz loop;
             zin = min(2 rb + 1, nb_z) of them are inside the grid and run 2 rb + 1 trips of the dy loop each; yin = min(2 rb + 1, nb_y)
             of those are inside the grid: rows = zin * yin rows of bricks.  A row on a face of the shell (at most min(rows,
             2 (zin + yin)) of them) runs 2 rb + 1 trips of the bx loop, every other row 2.  An unbounded gate: R = rb_max, the whole grid.
  far, dense table by rows (dense_far: max_ring > 4)
             nothing when limit <= (1 - margin) * cell.  Else rings rho = 0 .. R of rows around the query's, one call of dense_far_row
             each: 1 + 8 + 16 + ... = (2 R + 1)^2 calls, each two or four table loads whatever its extent, with
               R = min(max_ring, the last rho before limit <= (rho - 1 - margin) * cell) = min(max_ring, ceil(limit / cell + margin) + 1).
             An unbounded gate: R = max_ring = the longest axis + 1, the whole grid.
  far, dense table by blocks (dense_far_blocks: 2 <= max_ring <= 4)
             9 blocks of 3 occupancy words and at most 9 rows: 108 touches, whatever the limit.
  far query  a query more than kFarCells = 1 024 cells outside the grid (icp_kernels.hpp: far_query) takes none of the above: nothing when
             the gate cannot reach the box, else every target point once: n_points touches, which `points` already counts.
`margin` is kCellMargin in both (the dense search's own g.margin is never larger).
Not counted: the linear probing behind a brick's hash slot (brick_lookup).  The table is at most half full, so a probe chain is a
few slots on average; the model counts a brick probed as one touch, however long its chain.
"""
import collections
import math

import numpy as np

CELL_MARGIN = np.float32(0.03)      # kIcpPlanMargin = kCellMargin
COORD_MAX = np.float32(70000.0)     # kIcpCoordMax
AXIS_CELLS = 60000.0                # kIcpAxisCells
CELL_MAX = np.float32(2.0 ** 60)    # kIcpCellMax: the largest cell a search is served with (Plan.served)
NEAR = 36

Tunables = collections.namedtuple("Tunables", "cell_cap wide_cells dense_max_cells adaptive_cell")
DEFAULT = Tunables(0.014, True, 1 << 28, True)
Plan = collections.namedtuple("Plan", "cell inv_cell origin dims max_ring index_kind bounded served")


def tunables_of(env):
    """What csrc/tunables.hpp reads from the environment, as far as the rule looks at it."""
    t = DEFAULT
    if env.get("RSREG_CELL_CAP") and float(env["RSREG_CELL_CAP"]) > 0:
        t = t._replace(cell_cap=float(env["RSREG_CELL_CAP"]))
    if env.get("RSREG_DENSE_MAX_CELLS") is not None:
        t = t._replace(dense_max_cells=int(env["RSREG_DENSE_MAX_CELLS"]))
    if env.get("RSREG_FORCE_HASH", "")[:1] == "1":
        t = t._replace(dense_max_cells=0)
    if env.get("RSREG_NO_WIDE_CELLS", "")[:1] == "1":
        t = t._replace(wide_cells=False)
    if env.get("RSREG_NO_ADAPTIVE_CELL", "")[:1] == "1":
        t = t._replace(adaptive_cell=False)
    return t


def cell_pos(p, origin, inv_cell):
    """(p - origin) * inv_cell, both steps rounded to float32 (records.hpp: cell_pos)."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        d = (np.asarray(p, np.float32) - np.asarray(origin, np.float32)).astype(np.float32)
        return (d * np.float32(inv_cell)).astype(np.float32)


def host_cell_coord(p, origin, inv_cell):
    """host_cell_coord = the device's cell_coord: floor, then fmaxf(-4) and fminf(70000) -- a NaN comes out as -4."""
    with np.errstate(invalid="ignore"):
        f = np.floor(cell_pos(p, origin, inv_cell))
        f = np.fmin(np.fmax(f, np.float32(-4.0)), COORD_MAX)
    return f.astype(np.int64)


def plan(mn, mx, nfin, max_dist, refine=1.0, tun=DEFAULT):
    """icp_grid_plan.  served: whether the grid is searched at all -- a cell of at most 2^60 m, a box no wider than a float along
    any axis, the cell of its maximum below cell_coord's clamp."""
    mn, mx = np.asarray(mn, np.float32), np.asarray(mx, np.float32)
    max_dist, refine = float(max_dist), float(refine)
    cap = tun.cell_cap * min(3.0, max(1.0, math.pow(1.0e6 / max(float(int(nfin)), 1.0e4), 0.28)))
    extent = max(0.0, *[float(mx[k]) - float(mn[k]) for k in range(3)])
    bounded = math.isfinite(max_dist) and max_dist > 0 and max_dist < 0.25 * extent + 1e-3
    if bounded:
        padded = max_dist * 1.04
        parts = min(max(1, int(math.ceil(padded / (cap * refine)))), 8)
        cell = padded / parts
        if tun.wide_cells and parts == 1 and cap * refine > padded:
            cell = cap * refine
    else:
        cell = cap * refine
    cell = max(cell, extent / AXIS_CELLS)
    cell = max(cell, 1e-6)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        cell32 = np.float32(cell)
        inv32 = np.float32(1.0) / cell32
    dims = tuple(int(host_cell_coord(mx[k], mn[k], inv32)) + 2 for k in range(3))
    with np.errstate(over="ignore"):
        spans = (mx - mn).astype(np.float32)
    served = bool(cell32 <= CELL_MAX) and bool(np.isfinite(spans).all()) and all(d - 2 < int(COORD_MAX) for d in dims)
    max_dim = max(dims)
    max_ring = max_dim + 1
    if math.isfinite(max_dist) and max_dist >= 0:
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            rings = np.ceil(np.float64(max_dist) / np.float64(cell32) + np.float64(CELL_MARGIN))
        if rings < float(max_dim + 1):
            max_ring = max(1, int(rings))
    padded_cells = (dims[0] + 2) * (dims[1] + 2) * (dims[2] + 2)
    kind = 1 if (padded_cells <= tun.dense_max_cells and int(nfin) + 4 < (1 << 28)) else 0
    return Plan(cell32, inv32, mn.copy(), dims, max_ring, kind, bounded, served)


def refine_factor(n_unique, n_cells):
    """icp_refine_factor."""
    if n_cells == 0:
        return 1.0
    per_cell = float(n_unique) / float(n_cells)
    if not per_cell > 14.0:
        return 1.0
    return max(0.2, math.sqrt(8.0 / per_cell))


def box_of(xyz):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    fin = xyz[np.isfinite(xyz).all(axis=1)]
    return fin.min(axis=0), fin.max(axis=0), len(fin)


def occupancy(xyz, p):
    """(distinct finite points, occupied cells) of a brick-hash build over plan p: what its refinement looks at.  Points are
    distinct by value (-0 = +0)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    fin = xyz[np.isfinite(xyz).all(axis=1)] + np.float32(0.0)
    pts = np.unique(fin, axis=0)
    cells = np.stack([host_cell_coord(pts[:, k], p.origin[k], p.inv_cell) for k in range(3)], axis=1)
    return len(pts), len(np.unique(cells, axis=0))


def plan_of(xyz, max_dist, tun=DEFAULT):
    """The plan of the index a target build ends with: icp_grid_plan, and for a brick hash whose cells are crowded the plan of its
    second pass (build_grid: adaptive_cell)."""
    mn, mx, nfin = box_of(xyz)
    p = plan(mn, mx, nfin, max_dist, 1.0, tun)
    if p.index_kind == 0 and tun.adaptive_cell:
        r = refine_factor(*occupancy(xyz, p))
        if r != 1.0:
            p = plan(mn, mx, nfin, max_dist, r, tun)
    return p


def far_search(p):
    """Which search beyond ring 1 a query over this plan can get into: "hash_shells", "dense_rows", "dense_blocks" or "none"
    (max_ring <= 1: the gate fits into ring 1)."""
    if p.max_ring <= 1:
        return "none"
    if p.index_kind == 0:
        return "hash_shells"
    return "dense_blocks" if p.max_ring <= 4 else "dense_rows"


def _cells_of(limit, cell):
    """limit / cell as a double; +inf where either says nothing usable."""
    cell = float(cell)
    if not (math.isfinite(limit) and math.isfinite(cell) and cell > 0):
        return math.inf
    return limit / cell


def far_bound(p, limit):
    """Upper bound on the far search's touches of one query anywhere (module docstring)."""
    kind = far_search(p)
    m = float(CELL_MARGIN)
    reach = _cells_of(float(limit), p.cell)
    if kind == "none" or reach <= 1.0 - m:
        return 0
    if kind == "dense_blocks":
        return 108
    if kind == "dense_rows":
        r = p.max_ring if not math.isfinite(reach) else min(p.max_ring, int(math.ceil(reach + m)) + 1)
        return (2 * r + 1) ** 2
    nb = [(d + 3) >> 2 for d in p.dims]
    rb_max = min(max(nb) - 1, (p.max_ring + 3) // 4 + 1)
    r = rb_max if not math.isfinite(reach) else min(rb_max, int(math.ceil((reach + m) / 4.0)) + 1)
    rb = np.arange(r + 1, dtype=np.float64)
    w = 2.0 * rb + 1.0
    zin, yin = np.minimum(w, nb[2]), np.minimum(w, nb[1])
    rows = zin * yin
    face = np.minimum(rows, 2.0 * (zin + yin))
    return int((w + zin * w + face * w + 2.0 * rows).sum())


def cost_bound(p, limit, n_points):
    """Upper bound on the touches of one search of one query anywhere: near + every point once + the seed + far."""
    return NEAR + int(n_points) + 1 + far_bound(p, limit)
