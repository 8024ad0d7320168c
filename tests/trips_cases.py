"""The inputs of tests/test_trips_cpu.py and tests/test_trips_gpu.py: clouds with more finite records than one launch of the
one-wave-per-query kernels has workgroups (k_knn_indices, k_normals, k_radius_count, k_normals_radius of csrc/filters.hip run
min(nfin, 65 536) workgroups with a grid-stride loop over the queries in cell order), so that a workgroup answers a second, third
and fourth query, and record ids pass 65 535.

The uniform generator is the one of tests/test_normals_gpu.py (copied, as tests/radius_cases.py does); every record gets a w, a
colour and padding bytes of its own (radius_cases.cloud).

  two_trips_piles      66 000 uniform records, then 300 exact copies of the box's minimum corner and 300 of its maximum corner:
                       n = nfin = 66 600.  The first pile lies in cell 0, the head of the cell order: its queries overfill the
                       256-element selection buffer in trip 1, and the same workgroups answer ordinary queries in trip 2.  The
                       second pile lies in the last cell: its queries run in trip 2, after an ordinary query.
  launch_edge_N        N = 65 535, 65 536, 65 537 finite uniform records and 1 500 non-finite ones (NaN and inf) spread through
                       the cloud: record ids pass 65 535 while nfin sits on either side of the launch cap.
  four_trips           nfin = 3 * 65 536 + 1: workgroup 0 makes four trips, every other one three.
"""
import functools

import numpy as np

import pointgrid_layout as G
import radius_cases

LAUNCH_CAP = 1 << 16     # workgroups of one launch: min(nfin, 1 << 16) in csrc/filters.hip
PILE = 300               # copies in a pile: more than the 256 elements of the selection buffer (kKnnBuf)
N_UNIFORM = 66000
N_HOLES = 1500
SEED = 1
NAMES = ("two_trips_piles", "launch_edge_65535", "launch_edge_65536", "launch_edge_65537", "four_trips")
NFIN = {"two_trips_piles": N_UNIFORM + 2 * PILE, "launch_edge_65535": 65535, "launch_edge_65536": 65536, "launch_edge_65537": 65537,
        "four_trips": 3 * LAUNCH_CAP + 1}
# the radii of the radius search per case: at 0.05 a few records of two_trips_piles have fewer than three neighbours, at 0.02 most
# (tests/test_trips_cpu.py holds both); the other cases take one radius each
RADII = {"two_trips_piles": (0.05, 0.02), "launch_edge_65537": (0.05,), "four_trips": (0.03,)}


def uniform(n, seed):
    rng = np.random.default_rng(seed)                       # (the generator of test_normals_gpu.py::_uniform)
    return (rng.random((n, 3)) * np.array([2.0, 1.5, 0.7]) + np.array([-1.0, -0.5, 0.4])).astype(np.float32)


def _with_holes(nfin, seed):
    """nfin finite uniform records and N_HOLES non-finite ones spread through the cloud: whole-NaN records and records whose y
    is +inf, as the "non_finite" input of test_normals_gpu.py mixes them."""
    n = nfin + N_HOLES
    rng = np.random.default_rng(seed + 100)
    holes = rng.choice(n, N_HOLES, replace=False)
    xyz = np.empty((n, 3), np.float32)
    fin = np.ones(n, bool)
    fin[holes] = False
    xyz[fin] = uniform(nfin, seed)
    xyz[holes] = uniform(N_HOLES, seed + 200)
    xyz[holes[:N_HOLES // 2]] = np.nan
    xyz[holes[N_HOLES // 2:], 1] = np.inf
    return xyz


@functools.lru_cache(maxsize=None)
def xyz(name):
    """(n, 3) float32, read-only."""
    if name == "two_trips_piles":
        u = uniform(N_UNIFORM, SEED)
        out = np.concatenate([u, np.repeat(u.min(axis=0)[None], PILE, axis=0), np.repeat(u.max(axis=0)[None], PILE, axis=0)])
    elif name.startswith("launch_edge_"):
        out = _with_holes(int(name.rsplit("_", 1)[1]), SEED + 1)
    else:
        assert name == "four_trips"
        out = uniform(NFIN[name], SEED + 2)
    out = np.ascontiguousarray(out, np.float32)
    out.setflags(write=False)
    return out


def piles():
    """(record indices of the pile at the minimum corner, of the pile at the maximum corner) of two_trips_piles."""
    return np.arange(N_UNIFORM, N_UNIFORM + PILE), np.arange(N_UNIFORM + PILE, N_UNIFORM + 2 * PILE)


@functools.lru_cache(maxsize=None)
def cloud(name):
    return radius_cases.cloud(xyz(name), seed=7)


def cell_order_positions(points, policy="knn", min_cell=0.0):
    """Where every finite record can stand in the cell-sorted array of the grid: (first, last) positions of its cell's run (the order
    inside a cell is the build's own), -1 for a non-finite record; and the layout."""
    points = np.asarray(points, np.float32)
    lay = G.layout_of(points, policy, min_cell)
    fin = np.isfinite(points).all(axis=1)
    c = G.cells_of(points[fin], lay).astype(np.int64)
    flat = (c[:, 2] * lay.dims[1] + c[:, 1]) * lay.dims[0] + c[:, 0]      # x fastest
    cells, inv, counts = np.unique(flat, return_inverse=True, return_counts=True)
    start = np.concatenate([[0], np.cumsum(counts)])
    first = np.full(len(points), -1, np.int64)
    last = np.full(len(points), -1, np.int64)
    first[fin] = start[inv.reshape(-1)]
    last[fin] = start[inv.reshape(-1) + 1] - 1
    return first, last, lay


def trips(nfin):
    """The largest number of queries one workgroup answers."""
    return -(-nfin // min(nfin, LAUNCH_CAP))
