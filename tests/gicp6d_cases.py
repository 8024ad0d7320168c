"""Shared pieces of the GICP6D tests (tests/test_gicp6d_cpu.py, tests/test_gicp6d_gpu.py, tests/test_gicp6d_cpp.py): the textured
plane on which colour decides the pose, with its reference alignments (computed once per process), and random coloured clouds.

THE SCENE.  A plane z = 0: a 45 x 45 grid at 1 cm spacing, every point jittered by up to +-3.5 mm in x and y (2 025 target
records), under a smooth, non-periodic colour field (each channel a different low-order polynomial of the position, 8 bits).  The
source is 1 500 of the target's records -- colours included -- moved by the inverse of the truth: 2 degrees about the plane's
normal and (2.7, -2.1) cm in the plane, nearly three grid steps.  Every covariance is the plane's own, I - (1 - eps) n n^T: the
plane-to-plane objective leaves the in-plane part of the pose to the correspondences, and nearest neighbours in x, y, z lock onto
the wrong grid points.  The colour weight is the class's parameter; the scene uses SCENE_WEIGHT.
"""
import functools

import numpy as np

import gicp6d_ref
import gicp_cases
import gicp_ref
import plane_ref

SCENE_WEIGHT = 0.3
SCENE_GATE = 0.05
SCENE_X = (0.0, 0.0, np.deg2rad(2.0), 0.027, -0.021, 0.0)


def ref_tables():
    """the float64 formula rounded to float32: what the library's tables are, to an ulp"""
    S, F = gicp6d_ref.tables64()
    return S.astype(np.float32), F.astype(np.float32)


def pack_rgb(r, g, b):
    return (np.asarray(r, np.uint32) << 16) | (np.asarray(g, np.uint32) << 8) | np.asarray(b, np.uint32)


class Scene:
    """tgt, src (float32 (n, 3)), rgba_t, rgba_s (uint32), cov_s, cov_t (float64 (n, 6)), truth (float64 4 x 4), prm"""


@functools.lru_cache(maxsize=None)
def scene():
    rng = np.random.default_rng(11)
    side, step = 45, 0.01
    gx, gy = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    xy = np.stack([gx.ravel(), gy.ravel()], axis=1) * step + rng.uniform(-0.0035, 0.0035, (side * side, 2))
    c = Scene()
    c.tgt = np.concatenate([xy, np.zeros((len(xy), 1))], axis=1).astype(np.float32)
    u, v = xy[:, 0] / (side * step), xy[:, 1] / (side * step)
    r = 255.0 * np.clip(0.10 + 0.80 * u, 0, 1)
    g = 255.0 * np.clip(0.10 + 0.80 * v, 0, 1)
    b = 255.0 * np.clip(0.15 + 0.70 * (0.5 * u * u + 0.5 * (1 - v) * u + 0.3 * v * v), 0, 1)
    c.rgba_t = pack_rgb(np.rint(r), np.rint(g), np.rint(b))
    pick = np.sort(rng.choice(len(xy), 1500, replace=False))
    c.truth = plane_ref.euler_matrix(np.array(SCENE_X)).astype(np.float64)
    inv = np.linalg.inv(c.truth)
    c.src = (c.tgt[pick].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    c.rgba_s = c.rgba_t[pick]
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (len(xy), 1))
    c.cov_t = gicp_cases.plane_covariances(nrm)
    c.cov_s = gicp_cases.plane_covariances(nrm[pick])
    c.prm = gicp_ref.Params(max_correspondence_distance=SCENE_GATE, **gicp_cases.TIGHT)
    return c


def scene_lab(tables=None):
    """(lab_s, lab_t) of the scene from the given tables (None: ref_tables)"""
    c = scene()
    S, F = tables if tables is not None else ref_tables()
    return gicp6d_ref.lab(S, F, c.rgba_s), gicp6d_ref.lab(S, F, c.rgba_t)


@functools.lru_cache(maxsize=None)
def scene_reference6():
    c = scene()
    ls, lt = scene_lab()
    return gicp6d_ref.gicp6d(c.src, c.tgt, ls, lt, c.cov_s, c.cov_t, SCENE_WEIGHT, None, c.prm, truth=c.truth)


@functools.lru_cache(maxsize=None)
def scene_reference3():
    c = scene()
    return gicp_ref.gicp(c.src, c.tgt, c.cov_s, c.cov_t, None, c.prm, truth=c.truth)


def rgb_cloud(xyz, rgba, stride=32):
    """a PointCloud of POINT_DTYPE records (stride 32) with the given positions and packed colours"""
    from rsreg_amd import POINT_DTYPE, PointCloud
    pts = np.zeros(len(xyz), POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["w"] = 1.0
    pts["rgba"] = rgba
    return PointCloud(pts, width=len(xyz), height=1, is_dense=bool(np.isfinite(xyz).all()))


def box_cloud(n, seed, box=(2.0, 1.5, 0.7)):
    """n uniform points of the box and n random colours: (xyz float32, lab' float32 in [0, 1] x [-1, 1]^2)"""
    rng = np.random.default_rng(seed)
    xyz = (rng.uniform(0, 1, (n, 3)) * np.array(box)).astype(np.float32)
    lab = np.stack([rng.uniform(0, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)], axis=1).astype(np.float32)
    return xyz, lab
