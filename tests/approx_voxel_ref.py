"""pcl::ApproximateVoxelGrid<PointXYZRGB>::filter in numpy and Python, written from the rules in include/rsreg.h
("pcl::ApproximateVoxelGrid") and from nothing else: independent of csrc/voxel_host.cpp, csrc/voxel.hip and oracle/icp_oracle.c.

Every float operation is a float32 numpy operation on float32 operands (one IEEE rounding each).  The cell indices and the
slots are computed for all records at once; the stream itself -- which voxel a slot holds, what a record flushes -- is a Python
loop over integers; the sums of a run are np.cumsum over its records in input order (an accumulate is sequential by definition,
tests/voxelgrid_ref.py holds it against a Python loop).

  * The stream: a history of 512 slots.  A record whose slot holds another voxel flushes that voxel's centroid to the output and
    takes the slot; at the end the occupied slots are flushed in slot order.
  * The centroid: the sums of x, y, z and of the r, g, b bytes (each converted to float first), from +0.0f on in input order,
    divided by (float)count; the colour is (int) of the three byte means packed r << 16 | g << 8 | b; w is 1.0f; everything else is zero.
  * A record with a non-finite x, y or z takes no part.
  * The cell index of a coordinate: c = floorf(x * inv) with inv = 1.0f / leaf; INT32_MIN when c is a NaN or outside
    [-2^31, 2^31), else the integer c.
  * The slot: (ix * 7171 + iy * 3079 + iz * 4231) mod 2^32, & 511.
"""
import numpy as np

F = np.float32
INT32_MIN = -2 ** 31
HIST = 512


def cell_index(coord, leaf):
    """float32 array, one leaf size -> int64 array of cell indices (the rule above)"""
    coord = np.asarray(coord, F)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        inv = F(1.0) / F(leaf)
        c = np.floor((coord * inv).astype(F))
        inside = (c >= F(-2147483648.0)) & (c < F(2147483648.0))         # (a NaN compares false)
    out = np.full(coord.shape, INT32_MIN, np.int64)
    out[inside] = c[inside].astype(np.int64)
    return out


def slot_of(ix, iy, iz):
    """int64 arrays of cell indices -> the slot of the history"""
    u = lambda v: np.asarray(v, np.int64).astype(np.uint64) & np.uint64(0xffffffff)     # the int32's bits
    h = (u(ix) * np.uint64(7171) + u(iy) * np.uint64(3079) + u(iz) * np.uint64(4231)) & np.uint64(0xffffffff)   # (32 x 13 bits: no overflow of 64)
    return (h & np.uint64(HIST - 1)).astype(np.int64)


def finite_rows(points):
    return np.isfinite(points["x"]) & np.isfinite(points["y"]) & np.isfinite(points["z"])


def cells(points, leaf):
    """(n, 3) int64 cell indices of all records (those of non-finite records mean nothing)"""
    leaf = np.asarray(leaf, F).reshape(3)
    assert (leaf > 0).all()
    with np.errstate(invalid="ignore"):
        return np.stack([cell_index(points[f], leaf[a]) for a, f in enumerate("xyz")], axis=1)


def runs(points, leaf):
    """The stream: a list of (voxel, member indices in input order), in the order the centroids are emitted."""
    ijk = cells(points, leaf)
    slot = slot_of(ijk[:, 0], ijk[:, 1], ijk[:, 2]).tolist()
    vox = [tuple(v) for v in ijk.tolist()]
    hist = [None] * HIST                                     # slot -> (voxel, [members])
    out = []
    for i in np.flatnonzero(finite_rows(points)).tolist():
        s, v = slot[i], vox[i]
        held = hist[s]
        if held is not None and held[0] != v:
            out.append(held)
            held = None
        if held is None:
            held = hist[s] = (v, [])
        held[1].append(i)
    out.extend(h for h in hist if h is not None)
    return [(v, np.asarray(m, np.int64)) for v, m in out]


def components(points):
    rgba = points["rgba"].astype(np.uint32)
    return {"x": points["x"].astype(F), "y": points["y"].astype(F), "z": points["z"].astype(F),
            "r": ((rgba >> 16) & 0xff).astype(F), "g": ((rgba >> 8) & 0xff).astype(F), "b": (rgba & 0xff).astype(F)}


def approx_voxel_grid(points, leaf, the_runs=None):
    """points: a structured array with x, y, z, w (float32) and rgba (uint32) among its fields; the output has the same dtype."""
    the_runs = runs(points, leaf) if the_runs is None else the_runs
    comps = components(points)
    out = np.zeros(len(the_runs), points.dtype)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for j, (_, members) in enumerate(the_runs):
            cnt = F(len(members))
            mean = {k: F(np.cumsum(np.r_[F(0.0), v[members]], dtype=F)[-1] / cnt) for k, v in comps.items()}     # (a sum starts at +0.0f)
            rec = out[j:j + 1]
            rec["x"], rec["y"], rec["z"], rec["w"] = mean["x"], mean["y"], mean["z"], F(1.0)
            rec["rgba"] = (int(mean["r"]) << 16) | (int(mean["g"]) << 8) | int(mean["b"])
    return np.ascontiguousarray(out).view(np.uint8).copy().view(points.dtype)
