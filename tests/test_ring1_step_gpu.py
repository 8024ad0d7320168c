"""GPU: the ring-1 step of the dense-table search (csrc/icp_dense.hpp: dense_ring1_lane) -- which neighbour cell bit j of the
mask stands for, the three gaps its lower bound is added up from, the end it is read from, and where its entry lies in the
padded table (a 27-word table in LDS, filled by csrc/ring1_offsets.hpp: ring1_offset).  A wrong offset, a swapped axis or a
stride that went through a 24-bit multiply opens the wrong cell, and the nearest point is then missed.

The scenes are laid out in CELLS of the index that the library builds: the cell size is read back from rsreg_icp_grid_info
after a probe build with the same gate (it depends on the gate and on the cloud), the box is pinned by six points in the
middle of its faces, far from every query, and origin, cell size and dimensions are read back again from the build that is
searched.  Every point's cell is recomputed here the way the kernels do it (float32: (p - origin) * inv_cell) and checked.

Sites of a scene (each in cells of its own, four cells apart):
  * one neighbour at a time: for each j = dz * 9 + dy * 3 + dx except 13, a query 0.08 cells from the face, edge or corner it
    shares with neighbour j and one target point 0.04 cells beyond it -- and the same again with a farther point in the
    query's own cell, which the search finds first (the seed of the later launches);
  * all 26 neighbours and the own cell occupied, queries at the cell's eight corners, six face centres and centre;
  * queries whose own cell lies in each corner and on each face of the grid (the neighbours beyond are the table's border).
The scenes run on a grid whose three dimensions differ, and on a flat slab whose padded x and y dimensions multiply to more
than 2^23 (sxy of DenseDev: the z stride of the table), with the sites at its far end.  A fuzz of 2 000 x 2 000 random points
follows.

Every case goes through the staged search (unseeded, then seeded by its own result) against a float32 brute force that
follows FLANN's L2_Simple order with the lowest-index tie-break -- index and squared distance compared exactly -- and through
the fused kernels, unsplit and with every tile split over 2 / over 2 and 4 lanes per query (as tests/test_best_key_gpu.py:
three iterations bit for bit against the staged pipeline, one iteration's sums against the brute force's matches), with the
occupancy words built (RSREG_NO_NBR_FROM_TABLE=1) and with the default, under which a source of at most 65 536 points set
before a target whose gate fits into ring 1 gets an index without the words (kOccTab: the 0.013 gate on the small grids;
the slab is too large for the counting build that leaves them out, so it runs with the default alone)."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GATES = [0.013, 0.05, 1e30]
SCHED_KEYS = ("RSREG_SCHED", "RSREG_SCHED_MIN_TILES", "RSREG_SCHED_F2", "RSREG_SCHED_F4", "RSREG_SCHED_AT")
SPLIT2 = {"RSREG_SCHED": "1", "RSREG_SCHED_MIN_TILES": "1", "RSREG_SCHED_F2": "1.0", "RSREG_SCHED_F4": "0.0"}
SPLIT24 = {"RSREG_SCHED": "1", "RSREG_SCHED_MIN_TILES": "1", "RSREG_SCHED_F2": "0.5", "RSREG_SCHED_F4": "0.5"}
UNSPLIT = {"RSREG_SCHED": "0"}
WORDS = [{"RSREG_NO_NBR_FROM_TABLE": "1"}, {}]
ORIGIN = np.array([-1.5, 0.25, 2.0], np.float32)
N_PINS = 6
N_FILL = 400
_cells = {}
_brutes = {}


@pytest.fixture(scope="module")
def api(rs):
    from rsreg_amd import api as a, lib
    lib.build()
    if a.device_count() < 1:
        pytest.fail("no HIP device: the product has no CPU fallback")
    return a


def brute(key, src, tgt, gate):
    """tests/test_best_key_gpu.py's brute force (float32, (dx^2 + dy^2) + dz^2, first minimum, PCL's gate in double), once per scene and gate."""
    if key in _brutes:
        return _brutes[key]
    s, t = src.astype(np.float32), tgt.astype(np.float32)
    idx = np.full(len(s), -1, np.int64)
    d2o = np.zeros(len(s), np.float32)
    gate2 = float(gate) * float(gate)
    with np.errstate(over="ignore"):
        for i in range(len(s)):
            d = s[i] - t
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            j = int(np.argmin(d2))
            if not (float(d2[j]) > gate2):
                idx[i] = j
                d2o[i] = d2[j]
    _brutes[key] = (idx, d2o)
    return _brutes[key]


def _set_env(monkeypatch, env):
    for k in SCHED_KEYS + ("RSREG_NO_NBR_FROM_TABLE",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _new_icp(api, sc, tc, pipeline, iters, gate):
    icp = api.IterativeClosestPoint(api.Context(0))   # (a new context reads the environment again)
    icp.params = api.icp_params(max_iterations=iters, criteria_mode=1, pipeline_mode=pipeline, max_correspondence_distance=gate)
    icp.setInputSource(sc)   # the source first: what lets a small source's target leave the occupancy words out
    icp.setInputTarget(tc)
    return icp


def _result(icp, out):
    r = icp.result
    return (bytes(r.transform), bytes(r.sums_last), r.n_correspondences, r.iterations, r.state, r.converged, r.mse,
            np.stack([out.points[k] for k in "xyz"]).tobytes())


def check_all_forms(api, rs, monkeypatch, key, src, tgt, gate, words, grid=None):
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    want_idx, want_d2 = brute(key, src, tgt, gate)
    hit = want_idx >= 0
    sc, tc = rs.PointCloud.from_xyz(src), rs.PointCloud.from_xyz(tgt)

    # ---- the staged search: unseeded, then seeded
    _set_env(monkeypatch, dict(UNSPLIT, **words))
    icp = _new_icp(api, sc, tc, 0, 3, gate)
    icp.begin()
    gi = icp.grid_info()
    assert gi.index_kind == 1   # the dense table
    if grid is not None:        # the grid the scene was laid out for
        assert np.float32(gi.cell_size) == grid["cell"] and tuple(gi.dims) == grid["dims"] and (np.array(gi.origin, np.float32) == ORIGIN).all(), \
            (gi.cell_size, tuple(gi.dims), tuple(gi.origin), grid)
    for seeded in (False, True):
        idx, d2 = icp.search()
        assert np.array_equal(idx.astype(np.int64), want_idx), ("staged", seeded, gate, np.nonzero(idx != want_idx)[0][:10])
        assert np.array_equal(d2[hit], want_d2[hit]), ("staged", seeded, gate)
    icp.end()
    staged3 = _result(icp, icp.align())

    # ---- what one iteration's 17 sums must hold (a[0] matches, a[4..6] their target points, a[16] their squared distances):
    # f64 sums of n terms added up in another order than numpy's, each within n * 2^-53 * sum(|terms|)
    n = len(src)
    t64, d64 = tgt[want_idx[hit]].astype(np.float64), want_d2[hit].astype(np.float64)
    want_q, want_d = t64.sum(0), d64.sum()
    tol_q, tol_d = n * 2.0 ** -53 * np.abs(t64).sum(0), n * 2.0 ** -53 * np.abs(d64).sum()

    # ---- the fused kernels
    for name, pipeline, env in (("fused 1", 1, UNSPLIT), ("fused 2", 2, UNSPLIT), ("split by 2", 2, SPLIT2), ("split by 2 and 4", 2, SPLIT24)):
        _set_env(monkeypatch, dict(env, **words))
        icp = _new_icp(api, sc, tc, pipeline, 3, gate)
        got3 = _result(icp, icp.align())
        split = env is not UNSPLIT
        if split:
            assert icp.result.n_scheduled_launches > 0, (name, "the schedule was not built")
        assert got3 == staged3, (name, gate)
        icp.params = api.icp_params(max_iterations=1, criteria_mode=1, pipeline_mode=pipeline, max_correspondence_distance=gate)
        icp.align()
        r = icp.result
        if split:
            assert r.n_scheduled_launches == r.n_nn_launches, (name, "the first launch ran unsplit")
        sums = np.array(r.sums_last, np.float64)
        print("%s gate %g words %s: matches %d (want %d), |dQ| %s (bound %s), dD %.3g (bound %.3g)" %
              (name, gate, bool(words), r.n_correspondences, int(hit.sum()), np.abs(sums[4:7] - want_q), tol_q, abs(sums[16] - want_d), tol_d))
        assert r.n_correspondences == int(hit.sum()) and sums[0] == float(hit.sum()), (name, gate)
        assert (np.abs(sums[4:7] - want_q) <= tol_q).all(), (name, gate)
        assert abs(sums[16] - want_d) <= tol_d, (name, gate)
    return want_idx, want_d2


# ---------------------------------------------------------------------------------------------- scenes laid out in cells

def probe_cell(api, rs, gate):
    """The cell size the library chooses for this gate (a cloud of fewer than 10^4 points, a box far wider than the gate)."""
    if gate not in _cells:
        pts = (ORIGIN + np.array([[0, 0, 0], [3.0, 2.0, 1.0]], np.float32)).astype(np.float32)
        icp = _new_icp(api, rs.PointCloud.from_xyz(pts[:1]), rs.PointCloud.from_xyz(pts), 0, 1, gate)
        icp.begin()
        _cells[gate] = np.float32(icp.grid_info().cell_size)
        icp.end()
    return _cells[gate]


def at(cell, c, f):
    """the point at fraction f of cell c, c and f per axis"""
    return (ORIGIN.astype(np.float64) + (np.asarray(c, np.float64) + np.asarray(f, np.float64)) * float(cell)).astype(np.float32)


def cell_of(cell, p):
    """the cell of a point as the kernels compute it: floor((p - origin) * inv_cell) in float32; and the fraction inside it"""
    inv = np.float32(1.0) / np.float32(cell)
    u = (np.asarray(p, np.float32) - ORIGIN) * inv
    c = np.floor(u)
    return c.astype(np.int64), u - c


def layout(cell, D):
    """Targets and queries of the sites on a grid whose points span D cells per axis (the library's grid then has D + 1: one
    more layer beyond the far pins).  Returns (tgt, src, checks): checks = (query, target it must match, offset of that target's
    cell from the query's) for the one-neighbour sites."""
    D = np.asarray(D)
    rng = np.random.default_rng(7)
    mid = D // 2
    tgt, src, checks = [], [], []
    # the pins: the middle of each face of the box; the far ones at 0.99 of cell D - 1 (every other point stays below 0.97)
    for k in range(3):
        for far in (False, True):
            c, f = mid.copy().astype(np.float64), np.full(3, 0.5)
            c[k], f[k] = (D[k] - 1, 0.99) if far else (0, 0.0)
            tgt.append(at(cell, c, f))
    assert len(tgt) == N_PINS
    # where the sites go: a lattice four cells apart, counted from the far end in x and y (large table indices)
    zs = [1] if D[2] < 7 else list(range(2, D[2] - 2, 4))
    sites = iter([(D[0] - 3 - 4 * a, D[1] - 3 - 4 * b, z) for z in zs for b in range(min((D[1] - 4) // 4, 8)) for a in range(min((D[0] - 4) // 4, 8))])
    # ---- one neighbour at a time, without and with a farther point in the own cell
    for own in (False, True):
        for j in range(27):
            if j == 13:
                continue
            c = np.array(next(sites))
            d = np.array([j % 3, (j // 3) % 3, j // 9])   # dx, dy, dz in 0..2
            qf = np.where(d == 0, 0.08, np.where(d == 2, 0.92, 0.5))
            tf = np.where(d == 0, 0.96, np.where(d == 2, 0.04, 0.5))
            checks.append((len(src), len(tgt), tuple(d - 1)))
            src.append(at(cell, c, qf))
            tgt.append(at(cell, c + d - 1, tf))
            if own:   # 0.28 cells from the query towards the middle of its cell: farther than the neighbour's point (at most 0.12 * sqrt(3))
                n = (d != 1).sum()
                tgt.append(at(cell, c, qf + np.where(d == 0, 0.28, np.where(d == 2, -0.28, 0.0)) / np.sqrt(n)))
    # ---- all 27 cells occupied, queries at the corners, face centres and centre of the own cell
    c = np.array(next(sites))
    for d in itertools.product(range(3), repeat=3):
        for _ in range(3):
            tgt.append(at(cell, c + np.array(d) - 1, rng.uniform(0.05, 0.95, 3)))
    for f in itertools.product((0.03, 0.5, 0.97), repeat=3):
        if sum(x != 0.5 for x in f) in (0, 1, 3):
            src.append(at(cell, c, f))
    # ---- own cells in the corners and on the faces of the library's grid (cells 0 and D of an axis; points live in 0 .. D - 1)
    edge = [(0, D[k]) for k in range(3)]
    quarter = D // 4
    border = list(itertools.product(*edge))
    for k in range(3):
        for e in edge[k]:
            s = list(quarter)
            s[k] = e
            border.append(tuple(s))
    for c in border:
        c = np.array(c)
        for d in itertools.product(range(3), repeat=3):
            n = c + np.array(d) - 1
            if (n >= 0).all() and (n <= D - 1).all():
                for _ in range(2):
                    tgt.append(at(cell, n, rng.uniform(0.05, 0.95, 3)))
        for _ in range(3):
            src.append(at(cell, c, rng.uniform(0.05, 0.95, 3)))
    # ---- N_FILL more queries anywhere among the sites: more than one tile, so that the schedules have tiles to split
    lo = np.maximum(D - 36, 0)
    for _ in range(N_FILL):
        src.append(at(cell, lo, rng.uniform(0.0, 1.0, 3) * (D - lo)))
    return np.array(tgt, np.float32), np.array(src, np.float32), checks


def scene(api, rs, gate, D):
    cell = probe_cell(api, rs, gate)
    tgt, src, checks = layout(cell, D)
    # the box is the pins': no other point reaches it
    assert (tgt.min(0) == tgt[:N_PINS].min(0)).all() and (tgt.max(0) == tgt[:N_PINS].max(0)).all() and (tgt[:N_PINS].min(0) == ORIGIN).all()
    dims = tuple(int(x) for x in cell_of(cell, tgt.max(0))[0] + 2)   # icp.hip: dims = cell of the far corner + 2
    assert dims == tuple(int(x) + 1 for x in D), (dims, D)
    # every one-neighbour pair sits where it is meant to, by the kernels' own arithmetic, clear of the cell walls
    for qi, ti, off in checks:
        (qc, qf), (tc, tf) = cell_of(cell, src[qi]), cell_of(cell, tgt[ti])
        assert tuple(tc - qc) == off, (qi, ti, off, qc, tc)
        assert (qf > 0.02).all() and (qf < 0.98).all() and (tf > 0.01).all() and (tf < 0.99).all(), (qf, tf)
    return tgt, src, checks, {"cell": cell, "dims": dims}


def run_scene(api, rs, monkeypatch, gate, D, words, name):
    tgt, src, checks, grid = scene(api, rs, gate, D)
    idx, _ = check_all_forms(api, rs, monkeypatch, (name, gate), src, tgt, gate, words, grid)
    # the scene does what it is for: each one-neighbour query matches the point in neighbour j (the brute force says so too)
    for qi, ti, _ in checks:
        assert idx[qi] == ti, (qi, ti, idx[qi])
    if gate < 1.0:
        assert not ((idx[:-N_FILL] >= 0) & (idx[:-N_FILL] < N_PINS)).any()   # the pins are beyond the gate of every site's queries
    return grid


@pytest.mark.parametrize("words", WORDS, ids=["occupancy-words", "default"])
@pytest.mark.parametrize("gate", GATES)
def test_sites_on_a_grid_of_unequal_dimensions(api, rs, monkeypatch, gate, words):
    grid = run_scene(api, rs, monkeypatch, gate, (31, 23, 15), words, "unequal")
    assert len(set(grid["dims"])) == 3


@pytest.mark.parametrize("gate", GATES)
def test_sites_on_a_slab_whose_z_stride_exceeds_2_to_the_23(api, rs, monkeypatch, gate):
    grid = run_scene(api, rs, monkeypatch, gate, (4100, 2050, 3), {}, "slab")
    sx, sy = grid["dims"][0] + 2, grid["dims"][1] + 2   # the padded table's x and y dimensions: sx * sy = DenseDev's sxy
    assert sx * sy > 2 ** 23


@pytest.mark.parametrize("words", WORDS, ids=["occupancy-words", "default"])
@pytest.mark.parametrize("gate", GATES)
def test_fuzz(api, rs, monkeypatch, gate, words):
    """2 000 random targets, 2 000 random queries in a box of a few thousand cells: most queries open several neighbours."""
    rng = np.random.default_rng(8)
    tgt = rng.uniform(-0.3, 0.3, (2000, 3)).astype(np.float32)
    src = rng.uniform(-0.32, 0.32, (2000, 3)).astype(np.float32)
    idx, _ = check_all_forms(api, rs, monkeypatch, ("fuzz", gate), src, tgt, gate, words)
    assert (idx >= 0).sum() > (100 if gate < 0.02 else 1000)
