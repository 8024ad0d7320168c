"""The inputs of tests/test_radius_cpu.py and tests/test_radius_gpu.py: the generators of tests/test_normals_gpu.py, copied (that
file stays as it is), so the radius search is held against the same clouds as the k-NN search."""
import functools

import numpy as np

import sor_ref as S

H = 2.0 ** -6            # the lattice's step: every coordinate and every difference is exact in float32
R_AT = H                 # an inner lattice point's six face neighbours lie AT this radius: not neighbours
R_FACE = 1.0001 * H      # ... inside this one: 1 + 6
R_SQRT2 = float(np.sqrt(2) * H)   # r * r rounds to exactly 2 H^2 in float32: the twelve edge neighbours lie AT it
R_EDGE = 1.5 * H         # 1 + 6 + 12


def cloud(xyz, width=None, height=1, is_dense=False, seed=0):
    """Records with a colour, a w and padding bytes of their own each: nothing but x, y, z may enter a result, and a record that
    moved or lost a byte shows."""
    from rsreg_amd import POINT_DTYPE, PointCloud
    rng = np.random.default_rng(seed)
    pts = np.zeros(len(xyz), POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["w"] = rng.random(len(xyz)).astype(np.float32)
    pts["rgba"] = rng.integers(0, 2 ** 32, len(xyz), dtype=np.uint32)
    pts.view(np.uint8).reshape(len(xyz), 32)[:, 20:] = rng.integers(0, 256, (len(xyz), 12), dtype=np.uint8)   # (the padding travels too)
    return PointCloud(pts, width=len(xyz) if width is None else width, height=height, is_dense=is_dense)


def lattice(m):
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)
    return (g * H + np.array([0.0, 0.0, 1.0])).astype(np.float32)


def uniform(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * np.array([2.0, 1.5, 0.7]) + np.array([-1.0, -0.5, 0.4])).astype(np.float32)


def sphere(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = 0.5 + 0.002 * rng.standard_normal(n)
    return (np.array([0.1, -0.2, 1.5]) + r[:, None] * u).astype(np.float32)


def non_finite_xyz():
    rng = np.random.default_rng(4)
    xyz = uniform(3000, 5)
    xyz[rng.integers(0, 3000, 150)] = np.nan
    xyz[rng.integers(0, 3000, 150), 1] = np.inf
    return xyz


@functools.lru_cache(maxsize=None)
def input_cloud(name):
    from rsreg_amd import PointCloud, synth
    if name == "lattice":
        return cloud(lattice(12))
    if name == "lattice_copies64":                          # point 777 and 63 copies of it behind the lattice: a pile of exactly 64
        xyz = lattice(12)
        return cloud(np.concatenate([xyz, np.repeat(xyz[777][None], 63, axis=0)]))
    if name == "lattice_pile":                              # 300 copies: one cell's run is longer than a wave
        xyz = lattice(12)
        return cloud(np.concatenate([xyz, np.repeat(xyz[777][None], 300, axis=0)]))
    if name == "uniform1000":
        return cloud(uniform(1000, 1))
    if name == "uniform5000":
        return cloud(uniform(5000, 2))
    if name == "sphere5000":
        return cloud(sphere(5000, 3))
    if name == "non_finite":
        return cloud(non_finite_xyz(), width=60, height=50)
    if name == "one":
        xyz = np.full((9, 3), np.nan, np.float32)
        xyz[4] = (0.25, -1.0, 2.0)
        return cloud(xyz)
    if name == "none_finite":
        xyz = np.full((70, 3), np.nan, np.float32)
        xyz[::3, 1] = np.inf
        return cloud(xyz)
    if name == "empty":
        return cloud(np.zeros((0, 3), np.float32))
    fr = synth.render_frame(1, "50k")                        # raw: the missing-depth records, thousands of them, at the origin
    if name == "frame_raw":
        return fr
    assert name == "frame_pass"
    pts = fr.points[S.passthrough_keep(fr.xyz, 2, 0.2, 2.5)]
    return PointCloud(np.ascontiguousarray(pts), width=len(pts), height=1, is_dense=True)
