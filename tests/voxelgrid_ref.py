"""pcl::VoxelGrid<PointXYZRGB>::filter in numpy, written from the contract in include/rsreg.h ("pcl::VoxelGrid") and from
nothing else: independent of csrc/voxel_host.cpp and of csrc/voxel.hip.

Every operation is a float32 numpy operation on float32 operands (one IEEE rounding each).  The sums of a leaf are
np.cumsum over the leaf's points in ascending input index: an accumulate is sequential by definition (out[i] = out[i-1] + a[i]),
unlike np.sum, whose pairwise order is a different float sum.  sequential_sum() is the same sum spelled as a Python loop; the
CPU tests hold the two against each other.
"""
import numpy as np

INT32_MAX = 2 ** 31 - 1
F = np.float32


def sat_i32(v):
    """float32 array -> int64 array holding the saturated int32 conversion of the contract"""
    v = np.asarray(v, F)
    out = np.empty(v.shape, np.int64)
    hi, lo = v >= F(2147483648.0), v <= F(-2147483648.0)
    mid = ~(hi | lo)
    out[hi], out[lo] = INT32_MAX, -INT32_MAX - 1
    out[mid] = np.trunc(v[mid]).astype(np.int64)
    return out


def raw_copy(records):
    """a copy of the records byte for byte (ndarray.copy() of a padded structured dtype leaves the padding undefined)"""
    return np.ascontiguousarray(records).view(np.uint8).copy().view(records.dtype)


def sequential_sum(values):
    acc = F(0.0)
    for v in np.asarray(values, F):
        acc = F(acc + v)
    return acc


def finite_rows(points):
    return np.isfinite(points["x"]) & np.isfinite(points["y"]) & np.isfinite(points["z"])


def wrap_i32(v):
    """Python int -> the int32 with the same low 32 bits"""
    v &= 0xffffffff
    return v - (1 << 32) if v >= (1 << 31) else v


def leaf_grid(points, leaf):
    """(info dict, idx of the finite records as uint32, positions of the finite records); idx is None when the leaf is too small"""
    leaf = np.asarray(leaf, F).reshape(3)
    assert (leaf > 0).all() and np.isfinite(leaf).all()
    inv = F(1.0) / leaf
    assert np.isfinite(inv).all()
    fin = np.flatnonzero(finite_rows(points))
    info = {"min_b": [0, 0, 0], "max_b": [0, 0, 0], "div_b": [0, 0, 0], "divb_mul": [0, 0, 0], "n_finite": len(fin), "n_leaves": 0,
            "n_out": 0, "overflowed": 0}
    if len(fin) == 0:
        return info, np.zeros(0, np.uint32), fin
    xyz = np.stack([points["x"][fin], points["y"][fin], points["z"][fin]], axis=1).astype(F)
    min_p, max_p = xyz.min(axis=0), xyz.max(axis=0)
    with np.errstate(over="ignore"):
        ext = ((max_p - min_p).astype(F) * inv).astype(F)
    cells = 1
    for a in range(3):
        if not ext[a] < F(2147483648.0):
            cells = INT32_MAX + 1
            break
        cells *= int(ext[a]) + 1      # (int() truncates, like the int64 cast of a non-negative float)
    if cells > INT32_MAX:
        info["overflowed"] = 1
        info["n_out"] = len(points)
        return info, None, fin
    with np.errstate(over="ignore"):
        min_b = sat_i32(np.floor((min_p * inv).astype(F)))
        max_b = sat_i32(np.floor((max_p * inv).astype(F)))
    div_b = [wrap_i32(int(max_b[a]) - int(min_b[a]) + 1) for a in range(3)]
    mul = [1, div_b[0] & 0xffffffff, ((div_b[0] & 0xffffffff) * (div_b[1] & 0xffffffff)) & 0xffffffff]
    info["min_b"], info["max_b"], info["div_b"] = [int(v) for v in min_b], [int(v) for v in max_b], div_b
    info["divb_mul"] = [wrap_i32(m) for m in mul]
    idx = np.zeros(len(fin), np.uint64)
    with np.errstate(over="ignore"):
        for a in range(3):
            rel = (np.floor((xyz[:, a] * inv[a]).astype(F)) - F(min_b[a])).astype(F)
            ijk = sat_i32(rel).astype(np.uint64) & np.uint64(0xffffffff)       # the int32's bits as an unsigned value
            idx = (idx + ijk * np.uint64(mul[a])) & np.uint64(0xffffffff)     # (32 x 32 bits: no overflow of 64)
    return info, idx.astype(np.uint32), fin


def voxel_grid(points, leaf, downsample_all_data=True, min_points=0, reverse_leaves=False):
    """(output records, info dict).  points: a structured array with x, y, z (float32) and rgba (uint32) among its fields; the
    output has the same dtype.  reverse_leaves: add every leaf's points in DESCENDING input index -- not the contract; the tests
    use it to show that their clouds tell the two orders apart."""
    info, idx, fin = leaf_grid(points, leaf)
    if idx is None:
        return raw_copy(points), info
    order = np.argsort(idx, kind="stable")
    sidx, spos = idx[order], fin[order]
    starts = np.flatnonzero(np.r_[True, sidx[1:] != sidx[:-1]]) if len(sidx) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(sidx)]
    info["n_leaves"] = len(starts)
    rgba = points["rgba"].astype(np.uint32)
    comps = {"x": points["x"].astype(F), "y": points["y"].astype(F), "z": points["z"].astype(F),
             "r": ((rgba >> 16) & 0xff).astype(F), "g": ((rgba >> 8) & 0xff).astype(F), "b": (rgba & 0xff).astype(F),
             "a": ((rgba >> 24) & 0xff).astype(F)}
    out = np.zeros(len(starts), points.dtype)
    kept = 0
    for s, e in zip(starts, ends):
        n = int(e - s)
        if n < min_points:
            continue
        members = spos[s:e]
        if reverse_leaves:
            members = members[::-1]
        cnt = F(n)
        mean = {k: F(np.cumsum(np.r_[F(0.0), v[members]], dtype=F)[-1] / cnt) for k, v in comps.items()}     # (a sum starts at +0.0f: a leaf of -0.0f alone gives +0.0f)
        rec = out[kept:kept + 1]
        rec["x"], rec["y"], rec["z"] = mean["x"], mean["y"], mean["z"]
        rec.view(np.uint8).reshape(-1)[12:16] = np.frombuffer(F(1.0).tobytes(), np.uint8)
        if downsample_all_data:
            c = {k: int(np.uint32(mean[k])) for k in "rgba"}
            rec["rgba"] = ((c["a"] << 24) | (c["r"] << 16) | (c["g"] << 8) | c["b"]) & 0xffffffff
        else:
            rec["rgba"] = 0xff000000
        kept += 1
    info["n_out"] = kept
    return raw_copy(out[:kept]), info
