"""The inputs of tests/test_cloud_layouts_gpu.py: the same records laid out at any stride the C ABI takes (include/rsreg.h: 12-, 16-,
32- and 48-byte records, any multiple of 4 from 12 on), and the cloud of the ApproximateVoxelGrid case.

records(xyz, stride): the first 12 bytes of a record are x, y, z; every further word holds a value unique to (record, word) -- an
odd multiple of (16 * record + word) modulo 2^32, a bijection -- so a word that is dropped, swapped or taken from a neighbouring
record shows in a byte compare.  The value does not depend on the stride: word 3 (w) and word 4 (rgba) are the same at every stride
that has them, which is what lets an output's x, y, z, w, rgba be held against the stride-32 run.
"""
import functools

import numpy as np

import radius_cases

STRIDES = (12, 16, 20, 32, 48)          # every search and filter of csrc/filters.hip and csrc/iinormals.hip
RGB_STRIDES = (20, 32, 36, 48)          # entry points that need rgb at byte 16
QNAN = 0x7fc00000


class RawCloud:
    """What DeviceCloud.upload reads: points (a 1-D array of np.void records), width, height, is_dense."""

    def __init__(self, points, width, height, is_dense):
        self.points, self.width, self.height, self.is_dense = points, int(width), int(height), bool(is_dense)

    def __len__(self):
        return len(self.points)


def words(xyz, stride):
    """(n, stride / 4) uint32: the records as words."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    assert stride >= 12 and stride % 4 == 0 and stride <= 64
    n, nw = len(xyz), stride // 4
    out = np.empty((n, nw), np.uint32)
    out[:, :3] = xyz.view(np.uint32)
    rec = np.arange(n, dtype=np.uint64)
    for w in range(3, nw):
        v = (rec * np.uint64(16) + np.uint64(w)) * np.uint64(0x9E3779B1) + np.uint64(0x7F4A7C15)   # (below 2^64 for n < 2^28)
        out[:, w] = (v & np.uint64(0xffffffff)).astype(np.uint32)
    return out


def records(xyz, stride):
    """(n,) np.void records of `stride` bytes."""
    return np.ascontiguousarray(words(xyz, stride)).view(np.dtype((np.void, stride))).reshape(-1)


def raw_cloud(xyz, stride, width=None, height=1, is_dense=False):
    rec = records(xyz, stride)
    return RawCloud(rec, len(rec) if width is None else width, height, is_dense)


def as_words(rec):
    """The records of a np.void array (or the bytes of a download) as (n, stride / 4) uint32."""
    rec = np.ascontiguousarray(rec)
    return rec.view(np.uint8).reshape(len(rec), -1).view(np.uint32)


@functools.lru_cache(maxsize=None)
def non_finite_xyz():
    """The 60 x 50 "non_finite" cloud of tests/test_normals_gpu.py: 3 000 records, about 300 of them NaN or inf."""
    xyz = radius_cases.non_finite_xyz()
    xyz.setflags(write=False)
    return xyz


# ------------------------------------------------------------------------------------------------ ApproximateVoxelGrid
LEAF_POINTS = (1, 47, 48, 49, 1023, 1024, 1025, 5000)    # csrc/voxel.hip: one thread below kLongRun = 48, one wave below kHugeRun = 1 024
VOXEL_LEAF = 1.0
VOXEL_HOLES = 40


@functools.lru_cache(maxsize=None)
def voxel_xyz():
    """Leaf k holds LEAF_POINTS[k] points in the unit cube at x = k; the leaves are interleaved in input order, with VOXEL_HOLES
    non-finite records among them.  The leaves' slots in the filter's 512-slot history, (7171 ix + 3079 iy + 4231 iz) & 511 = 3 k,
    differ: no leaf is flushed before the end, each one is ONE run of all its points."""
    rng = np.random.default_rng(31)
    parts = [rng.uniform(0.05, 0.95, (m, 3)) + np.array([k, 0.0, 0.0]) for k, m in enumerate(LEAF_POINTS)]
    holes = rng.uniform(0.05, 0.95, (VOXEL_HOLES, 3))
    holes[:VOXEL_HOLES // 2] = np.nan
    holes[VOXEL_HOLES // 2:, 2] = np.inf
    xyz = np.concatenate(parts + [holes]).astype(np.float32)
    xyz = np.ascontiguousarray(xyz[rng.permutation(len(xyz))])
    xyz.setflags(write=False)
    return xyz
