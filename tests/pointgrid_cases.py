"""The scenes of tests/test_pointgrid_layout_cpu.py and tests/test_pointgrid_searches_gpu.py: clouds that are thin, far from the
origin, piled up in one place, or laid out in the cells of the grid the library builds for them -- where the point grid of
csrc/pointgrid.hpp picks its cell by another rule than the bisection, where the float rounding of a coordinate is a sizeable part
of a cell, and where the answer of a search lies across a face, an edge or a corner of the query's cell.

Every scene is float32, has a fixed seed and holds at most 4 000 records.  SCENES names, per scene, the rule that fixes the cell of
the k-NN grid (tests/pointgrid_layout.py: layout(...).branch) and the cells per axis it must come out with (None: not pinned).

cell_sites and cell_sites_500 are built in cells of the k-NN grid.  Six pins in the middle of the faces of a box with three
different edge lengths fix the origin, and with the number of records -- fixed up front, fillers make it up -- the cell: the layout
is known before a site is placed.  A site is a query, m - 1 records within 0.02 cells of it, and then
  "near":  the true (m + 1)-th neighbour 0.10 cells away across a face, an edge or a corner of the query's cell, and a decoy in the
           query's own cell at 0.30 cells;
  "skip":  the true neighbour 1.08 cells (per axis) away, two cells on, the cell between them empty; the decoy 1.30 cells (per axis)
           the other way, in the first shell: a walk that stops after the shell that filled its list returns the decoy;
  "tie":   the record across the face and the decoy at exactly the same float32 distance (a power of two along one axis), the one
           across the face with the lower record index: the search with indices must return that one.
m is 1, 9 or 63 (the contested neighbour is the last of k = 2, 10, 64) or 50 or 64 (the last that enters the mean over 50 or 64).
Each of the 26 directions occurs once as "near" and once as "skip"; the sites lie in the corners, on the faces and in the interior
of the grid, at least four cells apart.  Coordinates are rounded to float32 first and every placement is checked on the rounded
values (cells_of): a placement that fails means the scene is wrong, not the library.
"""
import collections
import functools
import itertools

import numpy as np

import pointgrid_layout as G
from fitness_ref import d2_f32

# name -> (the rule that fixes the k-NN grid's cell, its cells per axis or None)
SCENES = collections.OrderedDict([
    ("line_x", ("emax/4000", (4001, 2, 2))),
    ("line_y", ("emax/4000", (2, 4001, 2))),
    ("line_z", ("emax/4000", (2, 2, 4001))),
    ("slab", ("bisection", None)),
    ("far_box", ("big*1e-5", None)),
    ("far_lattice", ("big*1e-5", (2, 2, 2))),
    ("one_point_pile", ("emax==0", (2, 2, 2))),
    ("one_point_pile_origin", ("emax==0", (2, 2, 2))),
    ("cluster_and_outliers", ("bisection", None)),
    ("holes", ("big*1e-5", None)),
    ("cell_sites", ("bisection", None)),
    ("cell_sites_500", ("bisection", None)),
])
LATTICE_H = 2.0 ** -11          # far_lattice's step: 2 ulp of a float32 near 2048
LATTICE_AT = 2048.0
PILE_AT = (1.5, -0.75, 2.25)
SITES_N = 2800                   # records of cell_sites: fixed up front, so the cell is known before a site is placed
SITES_EDGES = (2.0, 1.4, 0.9)
SITES_M = (1, 9, 63, 50, 64)

Site = collections.namedtuple("Site", "kind direction m cell query true decoy delta")


def _line(axis, seed):
    rng = np.random.default_rng(seed)
    xyz = np.empty((1500, 3), np.float32)
    xyz[:] = np.float32([0.25, -0.5, 0.75])
    t = rng.random(1500)
    t[0], t[-1] = 0.0, 1.0                       # the ends are pinned
    xyz[:, axis] = t.astype(np.float32)
    return xyz


def _far_box(seed=11):
    rng = np.random.default_rng(seed)
    return (np.array([1000.0, -2000.0, 500.0]) + 0.6 * (rng.random((3000, 3)) - 0.5)).astype(np.float32)


def _far_lattice(seed=12):
    rng = np.random.default_rng(seed)
    return (LATTICE_AT + rng.integers(0, 40, (3000, 3)) * LATTICE_H).astype(np.float32)


def _cluster_and_outliers(seed=13):
    rng = np.random.default_rng(seed)
    cluster = np.array([0.3, 0.2, 0.1]) + 0.05 * rng.random((2000, 3))
    corners = 20.0 * np.array(list(itertools.product((-1.0, 1.0), repeat=3)))
    xyz = np.concatenate([cluster[:1000], corners[:4], cluster[1000:], corners[4:]])
    return xyz.astype(np.float32)


def _holes(seed=14):
    rng = np.random.default_rng(seed)
    xyz = _far_box()
    bad = rng.choice(3000, 70, replace=False)
    xyz[bad[40:]] = xyz[bad[40]]                 # a pile of 30 copies
    xyz[bad[:20]] = np.nan
    xyz[bad[20:30], 1] = np.inf
    xyz[bad[30:40], 2] = -np.inf
    return xyz


# ------------------------------------------------------------------------------------------------ cell_sites
def _site_plan():
    """[(kind, direction, m)]: 26 "near", 26 "skip", 6 "tie" along +-x, +-y, +-z."""
    dirs = [d for d in itertools.product((-1, 0, 1), repeat=3) if any(d)]
    plan = [("near", d) for d in dirs] + [("skip", d) for d in dirs]
    plan += [("tie", tuple(s if a == k else 0 for k in range(3))) for a in range(3) for s in (-1, 1)]
    out = []
    for i, (kind, d) in enumerate(plan):
        out.append((kind, d, (1, 9, 63)[i % 3] if kind == "tie" else SITES_M[i % len(SITES_M)]))
    return out


def _site_places():
    """58 places, per axis "lo", "hi" or a cell of the interior: the 8 corners, 3 on each of the 6 faces, 32 in the interior (a
    lattice of 4 cells)."""
    places = [tuple(c) for c in itertools.product(("lo", "hi"), repeat=3)]
    for a in range(3):
        for side in ("lo", "hi"):
            for j in range(3):
                mid = [10 + 6 * j, 10 + 4 * j]
                places.append(tuple(side if k == a else mid.pop(0) for k in range(3)))
    places += [(8 + 4 * i, 8 + 4 * j, 8 + 4 * l) for i in range(4) for j in range(4) for l in range(2)]
    return places


def _cell_sites(offset, seed):
    rng = np.random.default_rng(seed)
    offset = np.asarray(offset, np.float64)
    edges = np.asarray(SITES_EDGES, np.float64)
    pins = []
    for a in range(3):
        for s in (0.0, 1.0):
            p = offset + 0.5 * edges
            p[a] = offset[a] + s * edges[a]
            pins.append(p)
    pins = np.asarray(pins).astype(np.float32)
    lay = G.layout(pins.min(axis=0), pins.max(axis=0), SITES_N, "knn")
    dims = np.asarray(lay.dims)
    origin, cell = lay.origin.astype(np.float64), float(lay.cell)
    top = dims - 3                               # the last cell that lies inside the box along every axis

    def f32(u):                                  # cell units -> the float32 coordinates
        return (origin + np.asarray(u, np.float64) * cell).astype(np.float32)

    plan, places = _site_plan(), _site_places()
    assert len(plan) == len(places) == 58
    rows, sites = [p for p in pins], []
    for i, (kind, d, m) in enumerate(plan):
        d = np.asarray(d)
        toward, back = (2, 1) if kind == "skip" else (1, 0)     # cells the site reaches along / against its direction
        need_lo = np.where(d < 0, toward, np.where(d > 0, back, 0))
        need_hi = np.where(d > 0, toward, np.where(d < 0, back, 0))
        place = places[(7 * i) % len(places)]
        c = np.array([need_lo[k] if place[k] == "lo" else top[k] - need_hi[k] if place[k] == "hi" else place[k] for k in range(3)])
        q0 = len(rows)
        if kind == "tie":
            a = int(np.flatnonzero(d)[0])
            delta = 2.0 ** np.floor(np.log2(0.2 * cell))                      # a power of two in (0.1, 0.2] cells
            step = delta / 4.0
            face = origin[a] + (c[a] + (1 if d[a] > 0 else 0)) * cell
            u = c + 0.5
            q = f32(u).astype(np.float64)
            # the multiple of delta / 4 nearest the face on the query's side, at least 0.03 cells from it
            if d[a] > 0:
                q[a] = np.floor((face - 0.03 * cell) / step) * step
            else:
                q[a] = np.ceil((face + 0.03 * cell) / step) * step
            q = q.astype(np.float32)
            assert float(q[a]) % step == 0.0
            across, decoy = q.copy(), q.copy()
            across[a] = np.float32(float(q[a]) + d[a] * delta)
            decoy[a] = np.float32(float(q[a]) - d[a] * delta)
            assert float(across[a]) - float(q[a]) == d[a] * delta and float(q[a]) - float(decoy[a]) == d[a] * delta
            true_cell = c + d
        else:
            delta = 0.0
            u = c + np.where(d > 0, 0.96, np.where(d < 0, 0.04, 0.5))
            q = f32(u)
            if kind == "near":
                across = f32(u + d * (0.10 / np.sqrt((d * d).sum())))
                v = rng.standard_normal(3)
                v = np.where(d != 0, -d * np.abs(v), v)                        # into the query's own cell
                decoy = f32(u + 0.30 * v / np.linalg.norm(v))
                true_cell = c + d
            else:
                across = f32(u + 1.08 * d)
                decoy = f32(u - 1.30 * d)
                true_cell = c + 2 * d
        rows.append(q)
        for _ in range(m - 1):
            v = rng.standard_normal(3)
            rows.append(f32(((q.astype(np.float64) - origin) / cell) + 0.02 * rng.random() ** (1 / 3) * v / np.linalg.norm(v)))
        rows.append(across)
        rows.append(decoy)
        sites.append(Site(kind, tuple(int(x) for x in d), m, tuple(int(x) for x in c), q0, q0 + m, q0 + m + 1, float(delta)))
        got = G.cells_of(np.asarray(rows[q0:]), lay)
        assert (got[:m] == c).all(), (i, kind, d, got[:m], c)
        assert (got[m] == true_cell).all(), (i, kind, d, got[m], true_cell)
        assert (got[m + 1] == (c - d if kind == "skip" else c)).all(), (i, kind, d, got[m + 1], c)
    site_cells = np.asarray([s.cell for s in sites])
    assert (np.abs(site_cells[:, None, :] - site_cells[None, :, :]).max(axis=2) + 4 * np.eye(len(sites), dtype=int) >= 4).all()
    assert (np.abs(G.cells_of(pins, lay)[:, None, :] - site_cells[None, :, :]).max(axis=2) >= 4).all()
    n_fill = SITES_N - len(rows)
    assert n_fill >= 200, n_fill
    fill = []
    while len(fill) < n_fill:                    # fillers: inside the box, four cells or more from every site
        p = (offset + edges * (0.02 + 0.96 * rng.random(3))).astype(np.float32)
        if (np.abs(G.cells_of(p, lay)[None, :] - site_cells).max(axis=1) >= 4).all():
            fill.append(p)
    xyz = np.asarray(rows + fill, np.float32)
    assert len(xyz) == SITES_N and (G.layout_of(xyz, "knn")[:3] == lay[:3])
    return xyz, tuple(sites)


@functools.lru_cache(maxsize=None)
def _built(name):
    sites = ()
    if name.startswith("line_"):
        xyz = _line("xyz".index(name[-1]), 7 + "xyz".index(name[-1]))
    elif name == "slab":
        xyz = (np.random.default_rng(10).random((3000, 3)) * np.array([1.0, 1.0, 1e-4]) + np.array([0.5, -0.25, 1.0])).astype(np.float32)
    elif name == "far_box":
        xyz = _far_box()
    elif name == "far_lattice":
        xyz = _far_lattice()
    elif name == "one_point_pile":
        xyz = np.tile(np.float32(PILE_AT), (200, 1))
    elif name == "one_point_pile_origin":
        xyz = np.zeros((200, 3), np.float32)
    elif name == "cluster_and_outliers":
        xyz = _cluster_and_outliers()
    elif name == "holes":
        xyz = _holes()
    elif name == "cell_sites":
        xyz, sites = _cell_sites((-0.7, 0.3, 0.5), 15)
    elif name == "cell_sites_500":
        xyz, sites = _cell_sites((500.0, 500.0, 500.0), 16)
    else:
        raise KeyError(name)
    assert xyz.dtype == np.float32 and len(xyz) <= 4000
    xyz.setflags(write=False)
    return xyz, sites


def scene(name):
    """(n, 3) float32, read-only."""
    return _built(name)[0]


def sites(name):
    """The Site records of cell_sites / cell_sites_500 (record numbers of the query, the true neighbour and the decoy), else ()."""
    return _built(name)[1]


def finite_count(name):
    return int(np.isfinite(scene(name)).all(axis=1).sum())


# ------------------------------------------------------------------------------------------------ the radii of a radius search
def _just_above(r2):
    """A radius whose float32 square (float32 of the double r * r) is the float32 next above r2."""
    up = np.nextafter(np.float32(r2), np.float32(np.inf))
    r = float(np.sqrt(float(up)))
    while np.float32(r * r) < up:
        r = float(np.nextafter(r, np.inf))
    assert np.float32(r * r) == up
    return r


@functools.lru_cache(maxsize=None)
def radii(name):
    """((what, radius), ...), picked from the layout of the scene's radius grid:
      "small"  so small that the policy's own cell stays above it;
      "cell"   it becomes the cell;
      "big"    above twice the extent: two cells per axis, every finite record a neighbour of every other;
      "at"     (far_lattice, the tie sites) its float32 square is exactly a squared distance that occurs: those are NOT neighbours;
      "above"  the float32 square next above that one: they are."""
    mn, mx, nfin = G.box_of(scene(name))
    plain = G.layout(mn, mx, nfin, "radius")
    emax = float((mx.astype(np.float64) - mn.astype(np.float64)).max())
    out = [("small", float(plain.cell) / 8.0), ("cell", float(plain.cell) * 1.7), ("big", 2.5 * max(emax, float(plain.cell)))]
    at = None
    if name == "far_lattice":
        at = 3.0 * LATTICE_H                     # (3, 0, 0) and (2, 2, 1) steps
    elif sites(name):
        at = [s.delta for s in sites(name) if s.kind == "tie"][0]
    if at is not None:
        assert np.float32(at * at) == np.float32(at) * np.float32(at) and float(np.float32(at * at)) == at * at
        out += [("at", at), ("above", _just_above(at * at))]
    return tuple(out)


# ------------------------------------------------------------------------------------------------ the source of a fitness score
def fitness_source(name, seed=21, n=1000, gate=1e-3):
    """1 000 source records for an alignment against scene `name` as the target: records of the scene moved by dyadic offsets, records
    beyond each face, edge and corner of the target's box at 1, 100 and 10 000 cells of the fitness grid, and non-finite ones.
    far_lattice: every record stays on the lattice (a multiple of LATTICE_H) and more than `gate` from every target record, so that
    the alignment finds no correspondence, the transform stays the identity and every squared distance is a multiple of 2^-22."""
    rng = np.random.default_rng(seed)
    tgt = scene(name)
    fin = tgt[np.isfinite(tgt).all(axis=1)]
    lay = G.layout_of(tgt, "fit")
    cell = float(lay.cell)
    mn, mx = fin.min(axis=0).astype(np.float64), fin.max(axis=0).astype(np.float64)
    lattice = name == "far_lattice"
    step = LATTICE_H if lattice else 2.0 ** np.floor(np.log2(cell / 8.0))
    out = []
    dirs = [np.asarray(d, np.float64) for d in itertools.product((-1, 0, 1), repeat=3) if any(d)]
    for cells in (1.0, 100.0, 10000.0):          # beyond every face, edge and corner: 78 records
        for d in dirs:
            p = np.where(d > 0, mx + cells * cell, np.where(d < 0, mn - cells * cell, mn + (mx - mn) * rng.random(3)))
            out.append(np.round(p / step) * step if lattice else p)
    n_bad = 22
    while len(out) < n - n_bad:                  # records of the scene moved by a dyadic offset
        p = fin[rng.integers(len(fin))].astype(np.float64) + rng.integers(-6, 7, 3) * step
        if lattice:
            if float(d2_f32(p.astype(np.float32)[None, :], fin).min()) <= (1.5 * gate) ** 2:
                continue
        out.append(p)
    src = np.asarray(out).astype(np.float32)
    bad = np.full((n_bad, 3), np.nan, np.float32)
    bad[::3] = src[:8]
    bad[::3, 1] = np.inf
    bad[1::3] = src[8:15]
    bad[1::3, 2] = -np.inf
    src = np.concatenate([src[:500], bad, src[500:]])
    assert len(src) == n
    return src
