"""The clouds that take the two voxel filters (pcl::ApproximateVoxelGrid, pcl::VoxelGrid) to the edges of float32, and the helpers
that call their implementations.  tests/test_voxel_scale_cpu.py shows on the references what each cloud is there for;
tests/test_voxel_scale_gpu.py asks the kernels.  Every cloud comes from a fixed seed and is small: at most about 14 000 records.

  (a) SCALED   the run-class cloud and the boundary cloud of tests/voxelgrid_cases.py, cloud and leaf times 2^e
  (b) approx_cases() "cell_*"    cell indices at and past int32, leaves whose reciprocal is +inf or a denormal
  (c) approx_cases() "cancel_*"  runs whose sum crosses zero, lands on it and drops through binades (one voxel at INT32_MIN)
  (d) range_cases()              sums that overflow, stay denormal, leave the denormals; one large term in front of ones
  (e) grid_cases() "far_*" ...   VoxelGrid boxes far from the origin and wide, the extreme leaves

An approx case is (points, leaf); a grid case is (points, leaf, downsample_all_data, min_points).  References are computed once per
case and shared."""
import ctypes as C
import functools

import numpy as np

import approx_voxel_ref as A
import voxelgrid_cases as V
import voxelgrid_ref as R

F = np.float32
FLT_MAX = float(np.finfo(F).max)
FLT_MIN = float(np.finfo(F).tiny)                    # the smallest normal float
POINT20 = np.dtype({"names": ["x", "y", "z", "w", "rgba"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u4"], "offsets": [0, 4, 8, 12, 16],
                    "itemsize": 20})

# ------------------------------------------------------------------------------------------------ (a) scaled clouds
EXPONENTS = (-100, -40, 40, 100)                     # the candidates; tests/test_voxel_scale_cpu.py shows that all four are in the window
SCALED = {"run_classes": (V.run_classes, V.RUN_LEAF), "boundaries_l003": (V.boundaries, (0.03, 0.03, 0.03)),
          "boundaries_aniso": (V.boundaries, (0.01, 0.02, 0.05))}


def ldexp32(a, e):
    return np.ldexp(np.asarray(a, F), int(e)).astype(F)


def scaled(name, e):
    """(points, leaf) of a base cloud, both times 2^e (exact: a power of two)"""
    make, leaf = SCALED[name]
    pts = R.raw_copy(make())
    for f in "xyz":
        pts[f] = ldexp32(pts[f], e)
    pts.flags.writeable = False
    return pts, tuple(float(v) for v in ldexp32(np.asarray(leaf, F), e))


def moved(records, e):
    """output records at scale 1 -> what they are at 2^e: xyz moved by the power of two, w and rgba as they are"""
    out = R.raw_copy(records)
    for f in "xyz":
        out[f] = ldexp32(out[f], e)
    return out


# ------------------------------------------------------------------------------------------------ (b) cell indices at and past int32
PAST_INT32 = (2147483520.0, 2.0 ** 31, -2.0 ** 31, -2.0 ** 31 - 256.0, 3e9, -3e9, 1e30, -1e30, FLT_MAX, -FLT_MAX)


def _rgba(rng, n):
    return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def _mixed(rng, ordinary, special):
    """the two sets of rows interleaved at random (the order inside each set is kept)"""
    take = np.zeros(len(ordinary) + len(special), bool)
    take[rng.choice(len(take), len(special), replace=False)] = True
    xyz = np.empty((len(take), 3), F)
    xyz[take], xyz[~take] = special, ordinary
    return xyz


def cell_cloud(leaf, axes, seed):
    """Records with a coordinate whose cell index is at or past int32 on the given axes, four of each value, among 600 ordinary
    records of +-6 leaves (1 728 voxels on 512 slots).  The other coordinates of half of the special records lie in cell 0: with the
    cell index INT32_MIN they share the slot of the ordinary voxel with index 0 there, and the two keep flushing each other."""
    rng = np.random.default_rng(seed)
    ordinary = (rng.uniform(-6, 6, (600, 3)) * leaf).astype(F)
    ordinary[::40] = (rng.uniform(0.1, 0.9, (15, 3)) * leaf).astype(F)      # voxel (0, 0, 0): slot 0, that of (INT32_MIN, 0, 0) and of INT32_MIN thrice
    values = np.repeat(np.asarray(PAST_INT32, np.float64), 4)
    if leaf != 1.0:                                       # leaf 0.01: x ~ +-3e7 and down to where x / leaf meets 2^31
        values = np.repeat(np.asarray([3e7, -3e7, 3.0000002e7, -2.9999998e7, 2.2e7, -2.2e7, 2.1474836e7, -2.1474838e7]), 5)
    rng.shuffle(values)
    special = (rng.uniform(-4, 4, (len(values), 3)) * leaf).astype(F)
    special[::2] = (rng.uniform(0.2, 0.8, (len(special[::2]), 3)) * leaf).astype(F)
    for a in axes:
        special[:, a] = values.astype(F)
    xyz = _mixed(rng, ordinary, special)
    return V.make(xyz, _rgba(rng, len(xyz)), w=rng.random(len(xyz)).astype(F))


def inf_reciprocal_cloud(seed=31):
    """for a leaf of 2^-140 (1.0f / leaf = +inf): x * inv is a NaN at 0.0 and -0.0, +inf and -inf elsewhere"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-4, 4, (200, 3)).astype(F)
    xyz[::7, 0], xyz[3::11, 0], xyz[5::13, 1], xyz[2::17, 2] = 0.0, -0.0, 0.0, -0.0
    return V.make(xyz, _rgba(rng, len(xyz)))


def denormal_reciprocal_cloud(seed=32):
    """for a leaf of 3e38 (1.0f / leaf is a denormal): ordinary records and records at 1e38 scale, both signs"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-4, 4, (200, 3)).astype(F)
    far = rng.choice(200, 60, replace=False)
    xyz[far] = (rng.choice([-1.0, 1.0], (60, 3)) * rng.uniform(0.2e38, 3.3e38, (60, 3))).astype(F)
    return V.make(xyz, _rgba(rng, len(xyz)))


# ------------------------------------------------------------------------------------------------ (c) cancelling runs
def cancelling_run(n, zero_at, seed):
    """n records of one voxel under the x86 rule (leaf 1: |x| >= 2^31, y and z inside one cell), x alternating in sign around
    +-3e9 with magnitudes over eight binades.  The record in front of each index of zero_at is a large one and the record there
    takes the running float sum back to exactly zero."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, F)
    s = F(0.0)
    for i in range(n):
        sign = 1.0 if i % 2 == 0 else -1.0
        if i in zero_at:
            assert abs(float(s)) >= 2.0 ** 31
            t = F(-s)
        elif i + 1 in zero_at:
            t = F(sign * 2.0 ** 42 * rng.uniform(1.0, 2.0))
        else:
            t = F(sign * 3e9 * 2.0 ** rng.uniform(-0.48, 7.0))
        x[i] = t
        s = F(s + t)
    assert (np.abs(x) >= F(2.0 ** 31)).all()
    xyz = np.stack([x, rng.uniform(0.2, 0.8, n).astype(F), rng.uniform(0.2, 0.8, n).astype(F)], axis=1)
    # a few ordinary records of other slots among them: the run is emitted at the end, between theirs
    xyz = _mixed(rng, rng.uniform(1.0, 4.0, (12, 3)).astype(F), xyz)
    return V.make(xyz, _rgba(rng, len(xyz)))


CANCEL = {"cancel_5": (5, (3,), 41), "cancel_60": (60, (17, 40), 42), "cancel_1500": (1500, (700,), 43),
          "cancel_1500_window_ends_at_zero": (1500, (300, 1023), 44)}


@functools.lru_cache(maxsize=None)
def approx_cases():
    """(b) and (c): name -> (points, leaf)"""
    c = {}
    for k, (leaf, tag) in enumerate(((1.0, "l1"), (0.01, "l001"))):
        for j, (axes, name) in enumerate((((0,), "x"), ((1,), "y"), ((0, 1, 2), "xyz"))):
            c["cell_%s_%s" % (tag, name)] = (cell_cloud(leaf, axes, 100 + 10 * k + j), (leaf,) * 3)
    tiny = float(np.ldexp(1.0, -140))
    c["cell_leaf_2m140"] = (inf_reciprocal_cloud(), (tiny, tiny, tiny))
    c["cell_leaf_2m140_x_only"] = (inf_reciprocal_cloud(), (tiny, 1.0, 1.0))
    c["cell_leaf_3e38"] = (denormal_reciprocal_cloud(), (3e38, 3e38, 3e38))
    for name, (n, zero_at, seed) in CANCEL.items():
        c[name] = (cancelling_run(n, zero_at, seed), (1.0, 1.0, 1.0))
    for pts, _ in c.values():
        pts.flags.writeable = False
    return c


# ------------------------------------------------------------------------------------------------ (d) sums that leave the normal range
RANGE_LENGTHS = (3, 60, 1100)                        # the thread, the wave and the workgroup kernel
RANGE_KINDS = ("plus_3e38", "minus_3e38", "denormal_stays", "denormal_crosses", "one_1e30_then_ones")


def range_cloud(kind, n):
    """(points, leaf): n records of ONE voxel and leaf"""
    rng = np.random.default_rng(RANGE_KINDS.index(kind) * 10000 + n)
    if kind in ("plus_3e38", "minus_3e38"):          # cell 3 (-4) of a leaf of 2^126, whose reciprocal is normal; the sum is +-inf from the second term on
        xyz = rng.uniform(3.0e38, 3.3e38, (n, 3)) * (1.0 if kind == "plus_3e38" else -1.0)
        leaf = 2.0 ** 126
    elif kind == "denormal_stays":                    # 2^-141 .. 2^-139; 1 100 of them stay below 2^-126
        xyz = np.ldexp(rng.integers(256, 1024, (n, 3)).astype(np.float64), -149)
        leaf = 1.0
    elif kind == "denormal_crosses":                  # every term a denormal, the sum a normal float from about the middle of the run on
        xyz = np.ldexp(rng.uniform(0.5, 0.9, (n, 3)) * min(1.0, 3.0 / n) * 2.0 ** 23, -149)
        leaf = 1.0
    else:                                             # x: 1e30, then ones; y: the 1e30 in the middle; z: ordinary
        xyz = np.ones((n, 3))
        xyz[0, 0], xyz[n // 2, 1] = 1e30, 1e30
        xyz[:, 2] = rng.uniform(0.1, 0.9, n)
        leaf = 2e30
    return V.make(xyz.astype(F), _rgba(rng, n)), (leaf, leaf, leaf)


@functools.lru_cache(maxsize=None)
def range_cases():
    """name -> (points, leaf)"""
    c = {"%s_%d" % (kind, n): range_cloud(kind, n) for kind in RANGE_KINDS for n in RANGE_LENGTHS}
    for pts, _ in c.values():
        pts.flags.writeable = False
    return c


# ------------------------------------------------------------------------------------------------ (e) VoxelGrid: far and wide boxes
def far_box(values, axis, nan, seed):
    """30 records, the coordinate of `axis` one of the three values in turn (so the input order changes leaf with every record), the
    other two inside one cell of a leaf of 1; optionally a record with a NaN, so that the sort needs a sentinel"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0.2, 0.8, (30, 3)).astype(F)
    xyz[:, axis] = np.asarray(values, F)[np.arange(30) % 3]
    pts = V.make(xyz, _rgba(rng, 30))
    if nan:
        pts["z"][11] = np.nan
    return pts


FAR = {"far_1e9": (1e9, 1e9 + 256, 1e9 + 512), "far_plus_3e9": (3e9, 3e9 + 256, 3e9 + 512), "far_minus_3e9": (-3e9, -3e9 - 256, -3e9 - 512),
       "far_max_b_only": (2147483520.0, 2.0 ** 31, 2.0 ** 31 + 256)}


@functools.lru_cache(maxsize=None)
def grid_cases():
    """(e): name -> (points, leaf, downsample_all_data, min_points)"""
    c = {}
    one = (1.0, 1.0, 1.0)
    for k, (name, values) in enumerate(FAR.items()):
        for nan in (False, True):
            c[name + ("_nan" if nan else "")] = (far_box(values, 0, nan, 200 + k), one, 1, 0)
            if name in ("far_plus_3e9", "far_max_b_only"):
                c[name + "_y" + ("_nan" if nan else "")] = (far_box(values, 1, nan, 300 + k), one, 1, 0)
    for name in FAR:                                                  # downsample_all_data = 0 on each far box, with and without a sentinel
        c[name + "_xyz_only"] = (c[name + ("_nan" if name in ("far_plus_3e9", "far_1e9") else "")][0], one, 0, 0)
    c["far_minus_3e9_min2"] = (np.concatenate([c["far_minus_3e9"][0], far_box((-3e9 - 1024,) * 3, 0, False, 9)[:1]]), one, 1, 2)
    # the last division of x is one past div_b: float32(33554430 - (-1)) rounds up to 2^25 = div_b[0], a key of 26 bits where the
    # product of the divisions has 25
    rng = np.random.default_rng(77)
    xyz = rng.uniform(0.2, 0.8, (9, 3)).astype(F)
    xyz[:, 0] = np.asarray([33554430.0, -1.0, 5.0], F)[np.arange(9) % 3]
    c["last_division_rounds_up"] = (V.make(xyz, _rgba(rng, 9)), one, 1, 0)
    nan = R.raw_copy(c["last_division_rounds_up"][0])
    nan["y"][4] = np.nan
    c["last_division_rounds_up_nan"] = (nan, one, 1, 0)
    both = V.make(rng.uniform(-4, 4, (20, 3)).astype(F), _rgba(rng, 20))
    both["x"][3], both["x"][12], both["z"][7] = FLT_MAX, -FLT_MAX, np.nan
    c["plus_and_minus_flt_max"] = (both, one, 1, 0)                    # the extent is +inf: overflowed, the output is the input
    c["at_1e30_leaf_1e28"] = (V.make(rng.uniform(0.5e30, 1.5e30, (40, 3)).astype(F), _rgba(rng, 40)), (1e28,) * 3, 1, 0)
    smallest = float(np.ldexp(1.0, -127))                             # a denormal whose reciprocal 2^127 is finite
    c["leaf_2m127"] = (V.make(np.ldexp(rng.uniform(0, 6, (40, 3)), -127).astype(F), _rgba(rng, 40)), (smallest,) * 3, 1, 0)
    wide = rng.uniform(-4, 4, (40, 3))
    wide[::3] = rng.choice([-1.0, 1.0], (14, 3)) * rng.uniform(0.2e38, 1.6e38, (14, 3))
    c["leaf_flt_max"] = (V.make(wide.astype(F), _rgba(rng, 40)), (FLT_MAX,) * 3, 1, 0)
    zeros = rng.uniform(-4, 4, (20, 3)).astype(F)                     # a leaf that holds -0.0f alone on x and y: its sums start at +0.0f
    zeros[::5, :2] = -0.0
    zeros[::5, 2] = 0.5
    c["leaf_of_negative_zeros"] = (V.make(zeros, _rgba(rng, 20)), one, 1, 0)
    for case in c.values():
        case[0].flags.writeable = False
    return c


REFUSED_LEAVES = (float(np.ldexp(1.0, -128)), float(np.ldexp(1.0, -140)))       # their reciprocals are +inf


# ------------------------------------------------------------------------------------------------ references, once per case
@functools.lru_cache(maxsize=None)
def approx_runs(group, name, e=0):
    pts, leaf = approx_case(group, name, e)
    return A.runs(pts, leaf)


def approx_case(group, name, e=0):
    if group == "scaled":
        return scaled(name, e)
    return (approx_cases() if group == "cell" else range_cases())[name]


@functools.lru_cache(maxsize=None)
def approx_reference(group, name, e=0):
    pts, leaf = approx_case(group, name, e)
    out = A.approx_voxel_grid(pts, leaf, approx_runs(group, name, e))
    out.flags.writeable = False
    return out


def grid_case(group, name, e=0):
    if group == "scaled":
        return scaled(name, e) + (1, 0)
    if group == "range":
        return range_cases()[name] + (1, 0)
    return grid_cases()[name]


@functools.lru_cache(maxsize=None)
def grid_reference(group, name, e=0):
    pts, leaf, all_data, mp = grid_case(group, name, e)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        out, info = R.voxel_grid(pts, leaf, bool(all_data), mp)
    out.flags.writeable = False
    return out, info


def grid_runs(pts, leaf):
    """the leaves of the VoxelGrid reference as (leaf index, member indices in input order), in leaf order"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        info, idx, fin = R.leaf_grid(pts, leaf)
    if idx is None or len(idx) == 0:
        return []
    order = np.argsort(idx, kind="stable")
    sidx, spos = idx[order], fin[order]
    starts = np.flatnonzero(np.r_[True, sidx[1:] != sidx[:-1]])
    return [(int(sidx[s]), spos[s:e]) for s, e in zip(starts, np.r_[starts[1:], len(sidx)])]


def partial_sums(pts, the_runs, fields="xyz"):
    """every partial float sum of every run, one array per field and run"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return [np.cumsum(pts[f][m].astype(F), dtype=F) for _, m in the_runs for f in fields]


def is_denormal(a):
    a = np.abs(np.asarray(a, F))
    return (a > 0) & (a < F(FLT_MIN))


APPROX_ALL = ([("scaled", n, e) for n in SCALED for e in (0,) + EXPONENTS] + [("cell", n, 0) for n in approx_cases()] +
              [("range", n, 0) for n in range_cases()])
GRID_ALL = ([("scaled", n, e) for n in SCALED for e in (0,) + EXPONENTS] + [("range", n, 0) for n in range_cases()] +
            [("far", n, 0) for n in grid_cases()])


def label(case):
    return case[1] + ("" if case[0] != "scaled" else "_2e%d" % case[2])


# ------------------------------------------------------------------------------------------------ the implementations
def restride(pts, dtype):
    """the records with x, y, z, w, rgba at the same offsets and another stride; a payload behind the colour is filled with a pattern"""
    out = np.zeros(len(pts), dtype)
    for f in ("x", "y", "z", "w", "rgba"):
        out[f] = pts[f]
    if "extra" in dtype.names:
        out["extra"] = 0xdeadbeef
    return out


def same_fields(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)) for f in ("x", "y", "z", "w", "rgba"))


def approx_host(lib, pts, leaf):
    """rsreg_approx_voxel_grid, the sequential host filter"""
    src = R.raw_copy(np.ascontiguousarray(pts))
    out, n_out, lf = np.zeros_like(src), C.c_size_t(0), np.asarray(leaf, F)
    lib.check(lib.lib().rsreg_approx_voxel_grid(src.ctypes.data, len(src), src.dtype.itemsize, lf.ctypes.data, out.ctypes.data, C.byref(n_out)))
    return R.raw_copy(out[:n_out.value])


def approx_gpu_host_records(lib, ctx, pts, leaf):
    """rsreg_approx_voxel_grid_gpu"""
    src = R.raw_copy(np.ascontiguousarray(pts))
    out, n_out, lf = np.zeros_like(src), C.c_size_t(0), np.asarray(leaf, F)
    lib.check(lib.lib().rsreg_approx_voxel_grid_gpu(ctx.h, src.ctypes.data, len(src), src.dtype.itemsize, lf.ctypes.data, out.ctypes.data,
                                                    C.byref(n_out)), ctx.h)
    return R.raw_copy(out[:n_out.value])


def approx_gpu_cloud(lib, ctx, pts, leaf, asynchronous=False):
    """rsreg_cloud_filter, or rsreg_cloud_filter_async (a side scratch set and its stream) -> (records, (n, stride, width, height, is_dense))"""
    cin, cout = V.Handle(lib, ctx, pts, is_dense=0), V.Handle(lib, ctx)
    lf = np.asarray(leaf, F)
    call = lib.lib().rsreg_cloud_filter_async if asynchronous else lib.lib().rsreg_cloud_filter
    lib.check(call(ctx.h, cin.h, lf.ctypes.data, cout.h), ctx.h)
    meta = cout.info()
    out = cout.download(np.ascontiguousarray(pts).dtype)
    cout.close()
    cin.close()
    return out, meta
