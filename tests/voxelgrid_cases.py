"""The clouds the VoxelGrid tests run (CPU: the host restatement against tests/voxelgrid_ref.py; GPU: the kernels against both),
the smallest at which each part of the filter can go wrong, and the helpers that call the three implementations.

A case is (points, leaf, downsample_all_data, min_points).  References are computed once per case and shared (reference())."""
import ctypes as C
import functools

import numpy as np

import voxelgrid_ref as R

F = np.float32
POINT = np.dtype({"names": ["x", "y", "z", "w", "rgba"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u4"], "offsets": [0, 4, 8, 12, 16],
                  "itemsize": 32})
# the same record with 16 bytes of payload behind it (a stride that is not PointXYZRGB's)
POINT48 = np.dtype({"names": ["x", "y", "z", "w", "rgba", "extra"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u4", ("<u4", 7)],
                    "offsets": [0, 4, 8, 12, 16, 20], "itemsize": 48})

# points per leaf: both sides of the thread / wave threshold (48) and of the wave / workgroup threshold (1 024), one window
# (1 024) and one fetch (4 096) of the workgroup kernel and one point past each
RUN_LENGTHS = (1, 2, 47, 48, 49, 1023, 1024, 1025, 2049, 4096, 4097)
RUN_LEAF = (1.0, 1.0, 1024.0)


def make(xyz, rgba, dtype=POINT, w=1.0):
    pts = np.zeros(len(xyz), dtype)
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    pts["x"], pts["y"], pts["z"], pts["w"], pts["rgba"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], w, rgba
    return pts


@functools.lru_cache(maxsize=None)
def run_classes():
    """Leaf l holds RUN_LENGTHS[l] points and lies at x in [l, l + 1); the points of all leaves are interleaved at random, so
    only a stable sort adds a leaf's points in input order.  Full-mantissa coordinates, and in z (leaf 1 024) one term near
    1 000 among terms below 1: the float sums depend on the order."""
    rng = np.random.default_rng(20240917)
    leaf_of = np.repeat(np.arange(len(RUN_LENGTHS)), RUN_LENGTHS)
    rng.shuffle(leaf_of)
    n = len(leaf_of)
    xyz = rng.random((n, 3)).astype(F)
    xyz[:, 0] = (xyz[:, 0] * F(0.999) + leaf_of).astype(F)
    for l, cnt in enumerate(RUN_LENGTHS):
        members = np.flatnonzero(leaf_of == l)
        xyz[members[cnt // 3], 2] = F(1000.0) + F(l) * F(0.37)
    rgba = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)      # alpha bytes of every value
    pts = make(xyz, rgba, w=rng.random(n).astype(F))
    pts.flags.writeable = False
    return pts


@functools.lru_cache(maxsize=None)
def boundaries(seed=5):
    """Points exactly on multiples of the leaf (as float32 products), negative coordinates (floor and truncation differ), a
    negative min_b, exact copies, and points anywhere in between."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-9, 10, (700, 3))
    parts = []
    for leaf in ((0.01, 0.02, 0.05), (0.03, 0.03, 0.03), (0.25, 0.25, 0.25)):
        parts.append((k * np.asarray(leaf, F)).astype(F))
    parts.append((rng.random((900, 3)) * 0.9 - 0.45).astype(F))
    xyz = np.concatenate(parts)
    xyz = np.concatenate([xyz, xyz[rng.integers(0, len(xyz), 150)]])
    xyz = xyz[rng.permutation(len(xyz))]
    pts = make(xyz, rng.integers(0, 2 ** 32, len(xyz), dtype=np.uint64).astype(np.uint32))
    pts.flags.writeable = False
    return pts


def with_non_finite(pts, seed=9):
    rng = np.random.default_rng(seed)
    out = R.raw_copy(pts)
    where = rng.choice(len(out), max(3, len(out) // 25), replace=False)
    for j, i in enumerate(where):
        out[("x", "y", "z")[j % 3]][i] = (np.nan, np.inf, -np.inf)[(j // 3) % 3]
    return out


def box_cloud(lo, hi, extra=0, nan=False, seed=3):
    """a handful of points between the corners lo and hi (both among them)"""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([[np.full(3, lo)], [np.full(3, hi)], lo + rng.random((6 + extra, 3)) * (hi - lo), [np.full(3, hi)], [np.full(3, lo)]])
    pts = make(xyz.astype(F), rng.integers(0, 2 ** 32, len(xyz), dtype=np.uint64).astype(np.uint32))
    if nan:
        pts["y"][4] = np.nan
    return pts


@functools.lru_cache(maxsize=None)
def alpha_cloud():
    """One leaf of 70 000 points with r = a = 255 (255 * 70 000 > 2^24: the colour sum and the alpha sum round on the way) and a
    g that makes the rounding steps differ, among leaves with other alphas."""
    rng = np.random.default_rng(77)
    n_big = 70000
    big = rng.random((n_big, 3)).astype(F)
    big_rgba = (np.uint32(0xffff0000) | (rng.integers(200, 256, n_big).astype(np.uint32) << 8) | rng.integers(0, 256, n_big).astype(np.uint32))
    small = (rng.random((3000, 3)) * np.array([6.0, 1.0, 1.0]) + np.array([1.0, 0.0, 0.0])).astype(F)
    small_rgba = rng.integers(0, 2 ** 32, len(small), dtype=np.uint64).astype(np.uint32)
    xyz, rgba = np.concatenate([big, small]), np.concatenate([big_rgba, small_rgba])
    p = rng.permutation(len(xyz))
    pts = make(xyz[p], rgba[p])
    pts.flags.writeable = False
    return pts


def cases():
    """name -> (points, leaf, downsample_all_data, min_points)"""
    c = {}
    rc = run_classes()
    for mp in (0, 1, 2, 48, 5000):
        c["run_classes_min%d" % mp] = (rc, RUN_LEAF, 1, mp)
    c["run_classes_xyz_only"] = (rc, RUN_LEAF, 0, 0)
    b = boundaries()
    for name, leaf in (("aniso", (0.01, 0.02, 0.05)), ("l003", (0.03, 0.03, 0.03)), ("l025", (0.25, 0.25, 0.25)), ("l1", (1.0, 1.0, 1.0))):
        c["boundaries_" + name] = (b, leaf, 1, 0)
    c["non_finite_in_dense_cloud"] = (with_non_finite(b), (0.03, 0.03, 0.03), 1, 0)
    # 1290^3 = 2 146 689 000 leaves < 2^31: keys of 31 bits (with a non-finite record: a sentinel in bit 31)
    c["keys_31_bits"] = (box_cloud(0.0, 1289.5), (1.0, 1.0, 1.0), 1, 0)
    c["keys_31_bits_and_sentinel"] = (box_cloud(0.0, 1289.5, nan=True), (1.0, 1.0, 1.0), 1, 0)
    # one leaf further out on every axis: 1291^3 > INT32_MAX, the output is the input
    c["overflow_1291"] = (box_cloud(0.0, 1290.5, nan=True), (1.0, 1.0, 1.0), 1, 0)
    # d = 1290 per axis but div_b = 1291 (the box starts and ends inside a leaf): 1291^3 > 2^31, keys of 32 bits
    c["keys_32_bits"] = (box_cloud(0.6, 1290.4), (1.0, 1.0, 1.0), 1, 0)
    c["keys_32_bits_and_sentinel"] = (box_cloud(0.6, 1290.4, nan=True), (1.0, 1.0, 1.0), 1, 0)
    # two points 1 000 apart at a leaf of 0.001: along one axis 10^6 leaves; along all three 10^18, which only an int64 product sees
    two = make(np.array([[0.0, 0.0, 0.0], [1000.0, 0.0, 0.0], [0.0005, 0.0, 0.0]], F), np.array([1, 2, 3], np.uint32))
    c["two_points_1000_apart_x"] = (two, (0.001, 0.001, 0.001), 1, 0)
    diag = make(np.array([[0.0, 0.0, 0.0], [1000.0, 1000.0, 1000.0]], F), np.array([1, 2], np.uint32))
    c["two_points_1000_apart_xyz"] = (diag, (0.001, 0.001, 0.001), 1, 0)
    c["alpha_70000"] = (alpha_cloud(), (1.0, 1.0, 1.0), 1, 0)
    c["empty"] = (np.zeros(0, POINT), (0.1, 0.1, 0.1), 1, 0)
    c["one_point"] = (make(np.array([[-0.31, 2.5, 0.07]], F), np.array([0x80102030], np.uint32)), (0.1, 0.1, 0.1), 1, 0)
    nf = make(np.full((40, 3), np.nan, F), np.arange(40, dtype=np.uint32))
    nf["x"][::3], nf["y"][::3] = np.inf, 1.0
    c["all_non_finite"] = (nf, (0.1, 0.1, 0.1), 1, 0)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    pts, leaf, all_data, mp = cases()[name]
    out, info = R.voxel_grid(pts, leaf, bool(all_data), mp)
    out.flags.writeable = False
    return out, info


def info_dict(info):
    """rsreg_voxel_grid_info (ctypes) -> the dict tests/voxelgrid_ref.py returns"""
    return {"min_b": list(info.min_b), "max_b": list(info.max_b), "div_b": list(info.div_b), "divb_mul": list(info.divb_mul),
            "n_finite": info.n_finite, "n_leaves": info.n_leaves, "n_out": info.n_out, "overflowed": info.overflowed}


def params(lib, leaf, all_data, mp):
    p = lib.VoxelGridParams()
    lib.lib().rsreg_voxel_grid_params_default(C.byref(p))
    p.leaf[0], p.leaf[1], p.leaf[2] = [float(F(v)) for v in leaf]
    p.downsample_all_data, p.min_points_per_voxel = int(all_data), int(mp)
    return p


def run_host(lib, pts, leaf, all_data, mp, in_place=False):
    """rsreg_voxel_grid -> (records, info dict)"""
    pts = np.ascontiguousarray(pts)
    src = R.raw_copy(pts)
    out = src if in_place else np.zeros_like(src)
    n_out, info = C.c_size_t(0), lib.VoxelGridInfo()
    lf = np.asarray(leaf, F)
    lib.check(lib.lib().rsreg_voxel_grid(src.ctypes.data, len(src), src.dtype.itemsize, lf.ctypes.data, int(all_data), int(mp), out.ctypes.data,
                                         C.byref(n_out), C.byref(info)))
    if not in_place:
        assert src.tobytes() == pts.tobytes()      # (the input is read only)
    return R.raw_copy(out[: n_out.value]), info_dict(info)


def run_gpu_host_records(lib, ctx, pts, leaf, all_data, mp):
    """rsreg_voxel_grid_gpu -> (records, info dict)"""
    src = R.raw_copy(pts)
    out = np.zeros_like(src)
    n_out, info = C.c_size_t(0), lib.VoxelGridInfo()
    p = params(lib, leaf, all_data, mp)
    lib.check(lib.lib().rsreg_voxel_grid_gpu(ctx.h, src.ctypes.data, len(src), src.dtype.itemsize, C.byref(p), out.ctypes.data, C.byref(n_out),
                                             C.byref(info)), ctx.h)
    return R.raw_copy(out[: n_out.value]), info_dict(info)


class Handle:
    """a device cloud of records of any stride, through the C ABI (the Python layer's DeviceCloud downloads 32-byte records only)"""

    def __init__(self, lib, ctx, pts=None, width=None, height=1, is_dense=1):
        self.lib, self.ctx, self.h = lib, ctx, C.c_void_p()
        lib.check(lib.lib().rsreg_cloud_create(ctx.h, C.byref(self.h)), ctx.h)
        if pts is not None:
            pts = np.ascontiguousarray(pts)
            lib.check(lib.lib().rsreg_cloud_upload(self.h, pts.ctypes.data, len(pts), pts.dtype.itemsize, len(pts) if width is None else width,
                                                   height, is_dense), ctx.h)

    def info(self):
        n, s, w, h, d = C.c_size_t(0), C.c_size_t(0), C.c_uint32(0), C.c_uint32(0), C.c_int(0)
        self.lib.check(self.lib.lib().rsreg_cloud_info(self.h, C.byref(n), C.byref(s), C.byref(w), C.byref(h), C.byref(d)), self.ctx.h)
        return n.value, s.value, w.value, h.value, d.value

    def version(self):
        i, v = C.c_uint64(0), C.c_uint64(0)
        self.lib.check(self.lib.lib().rsreg_cloud_version(self.h, C.byref(i), C.byref(v)))
        return v.value

    def download(self, dtype):
        n, stride = self.info()[:2]
        assert n == 0 or stride == dtype.itemsize
        out = np.zeros(n, dtype)
        self.lib.check(self.lib.lib().rsreg_cloud_download(self.h, out.ctypes.data, n), self.ctx.h)
        return out

    def close(self):
        if self.h:
            self.lib.lib().rsreg_cloud_destroy(self.h)
            self.h = None


def run_gpu_cloud(lib, ctx, pts, leaf, all_data, mp, in_place=False, width=None, height=1, is_dense=1):
    """rsreg_cloud_voxel_grid -> (records, info dict, (n, stride, width, height, is_dense) of the output, versions before / after)"""
    cin = Handle(lib, ctx, pts, width, height, is_dense)
    cout = cin if in_place else Handle(lib, ctx)
    before = cout.version()
    info = lib.VoxelGridInfo()
    p = params(lib, leaf, all_data, mp)
    lib.check(lib.lib().rsreg_cloud_voxel_grid(ctx.h, cin.h, C.byref(p), cout.h, C.byref(info)), ctx.h)
    meta, after = cout.info(), cout.version()
    out = cout.download(np.ascontiguousarray(pts).dtype)
    cin.close()
    if not in_place:
        cout.close()
    return out, info_dict(info), meta, (before, after)
