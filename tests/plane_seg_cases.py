"""The inputs of the plane-segmentation tests (tests/test_plane_seg_cpu.py asserts on the reference what every case is FOR;
tests/test_plane_seg_gpu.py compares the device with the reference on them).  The constants mirror csrc/plane_seg_plan.hpp and
are held against the header itself by tests/cpp/plane_seg_plan_rule.cpp."""
import numpy as np

BLOCK, RECORDS_PER_LANE, CHUNK, MAX_GROUPS, TRIES = 256, 4, 64, 4096, 16
TILE = BLOCK * RECORDS_PER_LANE
FIRST_BATCH, MAX_BATCH = 256, 4096

SIGMA = 0.002          # the noise of a scene's planes, metres
THRESHOLD = 0.01
EXTENT = 2.0           # a scene fills a cube of this side


def plan(n, H):
    """csrc/plane_seg_plan.hpp: plane_plan, in Python integers"""
    tiles, chunks = -(-n // TILE), -(-H // CHUNK)
    per = min(max(-(-(tiles * chunks) // MAX_GROUPS), 1), chunks)
    return tiles, chunks, per, -(-chunks // per)


def batch(done, max_iterations):
    """csrc/plane_seg_plan.hpp: plane_batch"""
    cap = min(11 * max_iterations, 0x7ffffff0)
    if done >= cap:
        return 0
    b, start = FIRST_BATCH, 0
    while start + b <= done:
        start += b
        if b < MAX_BATCH:
            b *= 2
    return min(b, cap - done)


# ---- scene A: a noisy tilted plane through a cube of clutter
A_NORMAL = np.array([0.3, -0.2, 0.933], np.float64) / np.linalg.norm([0.3, -0.2, 0.933])
A_POINT = np.array([1.0, 1.0, 1.0])


def scene_a(fraction, seed=0, n=2000):
    """(xyz float32 (n, 3), on_plane bool): n * fraction records on the plane through A_POINT with normal A_NORMAL (sigma SIGMA along
    the normal, spread over a disc of radius EXTENT / 2 in the plane), the others uniform in the cube [0, EXTENT]^3; shuffled"""
    rng = np.random.default_rng(1000 + seed)
    m = int(round(n * fraction))
    e1 = np.cross(A_NORMAL, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(A_NORMAL, e1)
    rad, ang = 0.5 * EXTENT * np.sqrt(rng.uniform(size=m)), rng.uniform(0, 2 * np.pi, m)
    on = A_POINT + np.outer(rad * np.cos(ang), e1) + np.outer(rad * np.sin(ang), e2) + np.outer(rng.normal(0, SIGMA, m), A_NORMAL)
    off = rng.uniform(0, EXTENT, (n - m, 3))
    xyz = np.concatenate([on, off]).astype(np.float32)
    flag = np.arange(n) < m
    order = rng.permutation(n)
    return np.ascontiguousarray(xyz[order]), flag[order]


# ---- scene B: a wall (x = 0), a floor (z = 0) and clutter
def scene_b(seed=0, n_wall=1200, n_floor=600, n_clutter=200):
    """(xyz float32, label int: 0 wall, 1 floor, 2 clutter); shuffled"""
    rng = np.random.default_rng(2000 + seed)
    wall = np.stack([rng.normal(0, SIGMA, n_wall), rng.uniform(0, EXTENT, n_wall), rng.uniform(0, EXTENT, n_wall)], axis=1)
    floor = np.stack([rng.uniform(0, EXTENT, n_floor), rng.uniform(0, EXTENT, n_floor), rng.normal(0, SIGMA, n_floor)], axis=1)
    clutter = rng.uniform(0.1, EXTENT, (n_clutter, 3))
    xyz = np.concatenate([wall, floor, clutter]).astype(np.float32)
    label = np.repeat([0, 1, 2], [n_wall, n_floor, n_clutter])
    order = rng.permutation(len(xyz))
    return np.ascontiguousarray(xyz[order]), label[order]


AXIS_Z, EPS_10_DEG = (0.0, 0.0, 1.0), float(np.deg2rad(10.0))

# name -> (make() -> xyz, parameters)
SEGMENT_CASES = {
    "a60_s0": (lambda: scene_a(0.6, 0)[0], dict(distance_threshold=THRESHOLD, seed=0)),
    "a60_s1": (lambda: scene_a(0.6, 0)[0], dict(distance_threshold=THRESHOLD, seed=1)),
    "a60_s2": (lambda: scene_a(0.6, 0)[0], dict(distance_threshold=THRESHOLD, seed=2)),
    "a60_unrefined": (lambda: scene_a(0.6, 0)[0], dict(distance_threshold=THRESHOLD, seed=0, optimize_coefficients=0)),
    "a30_exhausts_50": (lambda: scene_a(0.3, 0)[0], dict(distance_threshold=THRESHOLD, seed=0)),
    "a30_1000": (lambda: scene_a(0.3, 0)[0], dict(distance_threshold=THRESHOLD, seed=0, max_iterations=1000)),
    "b_plain": (lambda: scene_b(0)[0], dict(distance_threshold=THRESHOLD, seed=0)),
    "b_axis_z": (lambda: scene_b(0)[0], dict(distance_threshold=THRESHOLD, seed=0, max_iterations=1000, axis=AXIS_Z, eps_angle=EPS_10_DEG)),
    "b_axis_z_s1": (lambda: scene_b(0)[0], dict(distance_threshold=THRESHOLD, seed=1, max_iterations=1000, axis=AXIS_Z, eps_angle=EPS_10_DEG)),
    "b_axis_skip_cap": (lambda: scene_b(0)[0], dict(distance_threshold=THRESHOLD, seed=0, max_iterations=50, axis=AXIS_Z, eps_angle=EPS_10_DEG)),
    "a60_shifted": (lambda: (scene_a(0.6, 0)[0] + np.float32(1e4)).astype(np.float32), dict(distance_threshold=THRESHOLD, seed=0)),
    "a60_scaled": (lambda: (scene_a(0.6, 0)[0] * np.float32(1e-3)).astype(np.float32), dict(distance_threshold=THRESHOLD * 1e-3, seed=0)),
    "collinear": (lambda: collinear(300), dict(distance_threshold=THRESHOLD, seed=0)),
    "threshold_0": (lambda: scene_a(0.6, 0)[0], dict(distance_threshold=0.0, seed=0)),
    "n2": (lambda: scene_a(0.6, 0)[0][:2], dict(distance_threshold=THRESHOLD, seed=0)),
    "n0": (lambda: np.zeros((0, 3), np.float32), dict(distance_threshold=THRESHOLD, seed=0)),
}


def collinear(n):
    """n records on the line t * (1, 2, 4), t an integer: every difference is an exact multiple of (1, 2, 4) and every cross product
    exactly zero in float32"""
    t = np.arange(n, dtype=np.float32) - np.float32(n // 2)
    return np.ascontiguousarray(np.stack([t, 2 * t, 4 * t], axis=1).astype(np.float32))


# ---- the clouds of the hypothesis tests: name -> (make() -> xyz, parameters of rsreg_cloud_plane_hypotheses)
def with_nans(fraction=0.3, seed=5, n=500):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    bad = rng.uniform(size=n) < fraction
    xyz[bad, rng.integers(0, 3, bad.sum())] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, bad.sum())]
    return xyz


def with_duplicates(seed=6, n=400):
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, (6, 3)).astype(np.float32)
    return np.ascontiguousarray(base[rng.integers(0, 6, n)])          # six distinct points: most tries draw a repeated point


HYPOTHESIS_CASES = {
    "nans": (with_nans, dict(seed=3)),
    "collinear": (lambda: collinear(300), dict(seed=0)),
    "duplicates": (with_duplicates, dict(seed=1)),
    "n3": (lambda: np.array([[0, 0, 0], [1, 0, 0.25], [0, 1, -0.5]], np.float32), dict(seed=2)),
    "n2": (lambda: np.array([[0, 0, 0], [1, 0, 0]], np.float32), dict(seed=2)),
    "axis": (lambda: scene_b(0)[0], dict(seed=0, axis=AXIS_Z, eps_angle=EPS_10_DEG)),
    "axis_oblique": (lambda: scene_a(0.6, 0)[0], dict(seed=4, axis=(0.3, -0.2, 0.9), eps_angle=0.35)),
}
HYPOTHESES = 200


# ---- the models and clouds of the counting tests
COUNT_N = (0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
COUNT_H = (0, 1, 63, 64, 65, 200)
COUNT_STRIDES = (12, 16, 32, 48)


def count_cloud(n, seed=11):
    """n records in [-1, 1]^3, every 17th with a NaN or an inf in one coordinate"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    specials = np.array([np.nan, np.inf, -np.inf], np.float32)
    for i in range(3, n, 17):
        xyz[i, i % 3] = specials[(i // 17) % 3]
    return xyz


def count_models(H, seed=12):
    """H models: random unit normals with an offset in [-0.5, 0.5], and among the first ones (as far as H reaches) a zero normal with
    a small and with a large offset, NaN and +-inf entries, denormal normals, a huge normal"""
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(H, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    m = np.concatenate([nrm, rng.uniform(-0.5, 0.5, (H, 1))], axis=1).astype(np.float32)
    tiny = np.float32(1e-42)
    special = np.array([[0, 0, 0, 0.001], [0, 0, 0, 5.0], [np.nan, 0, 1, 0], [0, 1, 0, np.nan], [np.inf, 0, 0, 0], [0, 0, 1, -np.inf],
                        [tiny, -tiny, tiny, 0], [tiny, 0, 0, 0.02], [3e38, 3e38, 0, 0], [0, 0, 1, 0]], np.float32)
    k = min(len(special), max(H - 1, 0))
    m[1:1 + k] = special[:k]
    return m


def threshold_records(t):
    """records at z = t rounded to float, one float below and one above (eight of each; x and y vary), for the model (0, 0, 1, 0)"""
    f = np.float32(t)
    zs = np.repeat(np.array([np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(np.inf))], np.float32), 8)
    xyz = np.zeros((24, 3), np.float32)
    xyz[:, 0], xyz[:, 1], xyz[:, 2] = np.arange(24), -np.arange(24), zs
    xyz[1::2, 2] = -xyz[1::2, 2]          # both sides of the plane
    return xyz


# ---- three blobs standing on a floor
def blobs_on_floor(seed=0):
    """(xyz float32, label: -1 floor, 0 .. 2 the blobs): a floor z = 0 (sigma 1 mm) sampled on a 4 cm lattice over 2 m x 2 m, and three
    blobs of 150 records each, uniform in 10 cm cubes that rest 1.5 cm above it, at least 60 cm apart"""
    rng = np.random.default_rng(3000 + seed)
    gx, gy = np.meshgrid(np.arange(0, 2.0, 0.04), np.arange(0, 2.0, 0.04))
    floor = np.stack([gx.ravel(), gy.ravel(), rng.normal(0, 0.001, gx.size)], axis=1)
    blobs, labels = [], []
    for k, c in enumerate(((0.4, 0.4), (1.0, 1.0), (1.6, 0.5))):
        p = rng.uniform(0, 0.1, (150, 3)) + np.array([c[0], c[1], 0.015])
        blobs.append(p)
        labels.append(np.full(150, k))
    xyz = np.concatenate([floor] + blobs).astype(np.float32)
    label = np.concatenate([np.full(len(floor), -1)] + labels)
    return xyz, label
