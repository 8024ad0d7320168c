"""The inputs of tests/test_clusters_cpu.py and tests/test_clusters_gpu.py: the clouds of tests/radius_cases.py (imported: the
clustering is held against the same clouds as the radius search it runs on) and two constructions of their own.

snake(rows, width, cut): `rows` rows of `width` points at step H = 2^-6 along x, the rows 2 H apart in y, z = 1.  Rows r and r + 1 are
joined by ONE connector point, H from the last point of both (at the high-x end after an even row, at the low-x end after an odd
one).  Every coordinate is a multiple of H below 2^4: exact in float32, and so is every difference.  At R_FACE = 1.0001 H a point is
joined to the next of its row and a connector to its two row ends (H away); the nearest other pairs are sqrt(2) H apart -- ONE
component whose graph diameter is about its size, the deep-tree case of a union-find.  At R_AT = H nothing is joined (the compare
is strict): every record a singleton.  cut = k leaves connector k out: rows 0 .. k with their k connectors, and the rest.  The
records are shuffled by a seeded permutation, so neither the record order nor the cell order follows the chain.

blobs(): six Gaussian blobs (sigma 0.01) of 400, 400, 400, 150, 40 and 7 points around centres 1 apart, and 60 isolated points 0.5
apart, shuffled.  At BLOB_TOL = 0.05 each blob is one component (asserted on the reference where the sizes are used): three equal
sizes for the tie rule, 60 singletons tied among themselves.
"""
import functools

import numpy as np

from radius_cases import H, R_AT, R_FACE, cloud, input_cloud as _radius_cloud  # noqa: F401

BLOB_SIZES = (400, 400, 400, 150, 40, 7)
BLOB_ISOLATED = 60
BLOB_TOL = 0.05
SNAKE_SMALL = (12, 16)
SNAKE_LARGE = (280, 256)      # 71 959 records: more than the 65 536 workgroups of a walk launch
SNAKE_CUT = 100


def snake_groups(rows, width, cut=None):
    """(xyz float32 (n, 3), group (n,)): the records in shuffled order and the component (0 or 1) each belongs to at R_FACE."""
    xs, ys, part = [], [], []
    for r in range(rows):
        xs.append(np.arange(width, dtype=np.float64) * H)
        ys.append(np.full(width, 2 * r * H))
        part.append(np.full(width, 0 if cut is None or r <= cut else 1))
        if r + 1 < rows and r != cut:
            xs.append(np.array([(width - 1) * H if r % 2 == 0 else 0.0]))
            ys.append(np.array([(2 * r + 1) * H]))
            part.append(np.array([0 if cut is None or r < cut else 1]))
    x, y, part = np.concatenate(xs), np.concatenate(ys), np.concatenate(part)
    xyz = np.stack([x, y, np.ones_like(x)], 1).astype(np.float32)
    perm = np.random.default_rng(rows * 1000 + width).permutation(len(xyz))
    return xyz[perm], part[perm]


def snake_sizes(rows, width, cut):
    """The two components' sizes with connector `cut` left out, from the construction."""
    return (cut + 1) * width + cut, (rows - cut - 1) * width + (rows - cut - 2)


def blobs_groups():
    rng = np.random.default_rng(11)
    xyz, group = [], []
    for b, m in enumerate(BLOB_SIZES):
        centre = np.array([float(b % 3), float(b // 3), 1.5])
        xyz.append(centre + 0.01 * rng.standard_normal((m, 3)))
        group.append(np.full(m, b))
    iso = np.stack([0.5 * np.arange(BLOB_ISOLATED) - 10.0, np.full(BLOB_ISOLATED, 5.0), np.full(BLOB_ISOLATED, 1.5)], 1)
    xyz.append(iso)
    group.append(len(BLOB_SIZES) + np.arange(BLOB_ISOLATED))
    xyz, group = np.concatenate(xyz).astype(np.float32), np.concatenate(group)
    perm = rng.permutation(len(xyz))
    return xyz[perm], group[perm]


@functools.lru_cache(maxsize=None)
def input_cloud(name):
    if name == "snake_small":
        return cloud(snake_groups(*SNAKE_SMALL)[0])
    if name == "snake_small_cut":
        return cloud(snake_groups(*SNAKE_SMALL, cut=4)[0])
    if name == "snake_large":
        return cloud(snake_groups(*SNAKE_LARGE)[0])
    if name == "snake_large_cut":
        return cloud(snake_groups(*SNAKE_LARGE, cut=SNAKE_CUT)[0])
    if name == "blobs":
        return cloud(blobs_groups()[0])
    return _radius_cloud(name)
