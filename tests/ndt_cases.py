"""Named, seeded inputs of tests/test_ndt_ref_cpu.py and tests/test_ndt_paths_gpu.py: each reaches a branch of the NDT target
build (csrc/ndt.hip: rsreg_ndt_set_target_device) or of the derivative pass (csrc/ndt_kernels.hpp: ndt_pass_body) that the
clouds of tests/test_ndt_gpu.py do not.  Built in the test process from fixed seeds; nothing is read from a file.

A grid case is a dict: name, tgt (n x 3 float32), res, degenerate (its smallest eigenvalue is 0 up to rounding: only such a
case may leave the floor rule to the sign of a rounding error), expect (the host-visible value that selects the branch:
div, n_leaves, occupied, n_finite, kept -- asserted on the reference's own numbers).
A pass case is a dict: name, tgt, res, src (n x 3 float32), pose (6 doubles), expect (n, n_vox, pairs where known), and
bad (the indices of its non-finite records) where it has some.
"""
import numpy as np

f32 = np.float32
NAN, INF = f32(np.nan), f32(np.inf)


def cluster(rng, leaf, n, res=1.0, spread=0.3):
    """n points inside leaf (i, j, k) of a grid of `res`, no nearer than (0.5 - spread) res to its faces."""
    c = (np.asarray(leaf, np.float64) + 0.5) * res
    return (c + rng.uniform(-spread, spread, (n, 3)) * res).astype(f32)


def _case(name, tgt, res, degenerate=False, **expect):
    return {"name": name, "tgt": np.ascontiguousarray(tgt, f32), "res": res, "degenerate": degenerate, "expect": expect}


def _keys(name, far):
    rng = np.random.default_rng(11)
    # min corner from the first cluster (leaf 0, 0, 0), max corner from one sentinel point in leaf (far - 1,) * 3
    tgt = np.concatenate([cluster(rng, (0, 0, 0), 40), cluster(rng, (3, 2, 1), 37), [[far - 0.5] * 3], [[NAN, 0.5, 0.5]],
                          [[0.25, 0.25, 0.25]]])
    return _case(name, tgt, 1.0, div=(far, far, far), n_leaves=far ** 3, kept=2)


def _occupied(name, n_occ, seed):
    """n_occ occupied leaves of a 16 x 16 x 9 box: every 9th holds 6..15 points (kept), one 256 and one 257, the others 1..5."""
    rng = np.random.default_rng(seed)
    cells = [(i, j, k) for k in range(9) for j in range(16) for i in range(16)]
    pick = sorted(rng.choice(len(cells) - 2, n_occ - 2, replace=False) + 1)
    pick = [0] + list(pick) + [len(cells) - 1]      # both corners of the box occupied: div is (16, 16, 9)
    parts, kept = [], 0
    for q, c in enumerate(pick):
        n = 256 if q == 40 else 257 if q == 41 else (6 + (q // 9) % 10 if q % 9 == 0 else 1 + q % 5)
        kept += n >= 6
        parts.append(cluster(rng, cells[c], n))
    tgt = np.concatenate(parts)
    return _case(name, tgt[rng.permutation(len(tgt))], 1.0, div=(16, 16, 9), occupied=n_occ, kept=kept)


def _runs():
    rng = np.random.default_rng(5)
    lens = [255, 256, 257, 4095, 4096, 4097, 6, 15, 16, 17]
    tgt = np.concatenate([cluster(rng, (2 * i, 0, 0), n) for i, n in enumerate(lens)])
    return _case("runs_on_the_block_stride", tgt[rng.permutation(len(tgt))], 1.0, occupied=len(lens), kept=len(lens), counts=lens)


def _min_points():
    rng = np.random.default_rng(6)
    counts = [7, 3, 6, 5, 5, 6, 4, 8, 1, 7, 2, 6]
    tgt = np.concatenate([cluster(rng, (i, 0, 0), n) for i, n in enumerate(counts)])
    return _case("min_points_interleaved", tgt[rng.permutation(len(tgt))], 1.0, occupied=12, kept=6, counts=[7, 6, 6, 8, 7, 6])


def _edges():
    """res 0.3: six points with x EXACTLY float32(k * 0.3) for k = -5 .. 5 (the float32 product with 1 / 0.3 lands on k or
    just under it), half of the k = 0 ones -0.0, and six interior points per leaf beside them so that the count of a kept voxel
    says which side the boundary points fell; records with one non-finite coordinate are dropped."""
    rng = np.random.default_rng(7)
    res, parts = 0.3, []
    for k in range(-5, 6):
        b = np.full((6, 3), 0.15, np.float64)
        b[:, 0] = float(f32(k * 0.3))
        b[:, 1:] += rng.uniform(-0.1, 0.1, (6, 2))
        b = b.astype(f32)
        if k == 0:
            b[:3, 0] = f32(-0.0)
        parts += [b, cluster(rng, (k, 0, 0), 6, res)]
    parts.append(cluster(rng, (-6, 0, 0), 6, res))
    parts.append(np.array([[NAN, 0.1, 0.1], [0.1, INF, 0.1], [0.1, 0.1, -INF], [NAN, NAN, NAN]], f32))
    tgt = np.concatenate(parts)
    return _case("binning_edges", tgt[rng.permutation(len(tgt))], res, n_finite=len(tgt) - 4)


def _few_leaves():
    rng = np.random.default_rng(8)
    tgt = np.concatenate([cluster(rng, (0, 0, 0), 9), cluster(rng, (5, 5, 5), 8), cluster(rng, (2, 3, 1), 6), cluster(rng, (4, 0, 2), 3)])
    return _case("few_leaves_fewer_points", tgt, 1.0, div=(6, 6, 6), n_leaves=216, n_finite=26, occupied=4, kept=3)


def _far():
    rng = np.random.default_rng(9)
    tgt = np.concatenate([cluster(rng, (4000, -2501, 900), 50, spread=0.2), cluster(rng, (4001, -2500, 901), 20, spread=0.2)])
    return _case("voxel_far_from_origin", tgt, 1.0, kept=2)


def _shape(name, pts, degenerate):
    rng = np.random.default_rng(10)
    tgt = np.concatenate([np.asarray(pts, np.float64) + [0.5, 0.5, 0.5], cluster(rng, (2, 0, 0), 12)])
    return _case(name, tgt, 1.0, degenerate, kept=2)


def grid_cases():
    d = 0.125
    flat = [[i * d, j * d, 0.0] for i in (-2, -1, 1, 2) for j in (-1, 0, 1)]
    line = [[i * d, 0.0, 0.0] for i in (-3, -2, -1, 1, 2, 3)]
    iso = [[d, 0, 0], [-d, 0, 0], [0, d, 0], [0, -d, 0], [0, 0, d], [0, 0, -d]]
    none = np.array([[NAN, 0, 0], [0, INF, 0], [0, 0, -INF], [NAN, NAN, NAN], [INF, 1, 2], [1, NAN, 2], [3, 4, NAN]], f32)
    return [
        _keys("keys32_div1290", 1290), _keys("keys64_div1291", 1291), _keys("keys64_far", 80001),
        _few_leaves(), _occupied("occupied_2048", 2048, 21), _occupied("occupied_2049", 2049, 22), _runs(), _min_points(), _edges(),
        _case("no_finite_point", none, 1.0, n_finite=0, kept=0), _far(),
        _shape("flat_exact", flat, True), _shape("collinear_exact", line, True), _shape("coincident", [[0.25, 0.25, 0.25]] * 6, True),
        _shape("isotropic", iso, False),
    ]


# ---- pass cases ---------------------------------------------------------------------------------------------------------------
POSE_GENERAL = [0.02, -0.03, 0.01, 0.03, -0.02, 0.04]
# just under, on and just over PCL's 10e-5, either sign, every angle slot taking part
POSE_SNAP_A = [0.01, 0.02, -0.01, 0.99e-4, -1e-4, 1.01e-4]
POSE_SNAP_B = [-0.01, 0.0, 0.02, -1.01e-4, 1e-4, -0.99e-4]
POSES = {"general": POSE_GENERAL, "snap_a": POSE_SNAP_A, "snap_b": POSE_SNAP_B}


def _spots(n_vox):
    """Every other leaf of a 6 x 6 x 4 block around the origin (coordinates stay small: float32 keeps its digits)."""
    return [(2 * i - 6, 2 * j - 6, 2 * k - 4) for k in range(4) for j in range(6) for i in range(6)][:n_vox]


def row_target(rng, n_vox):
    """n_vox voxels of 8 points, no two in adjacent leaves: a point near one of them is within the radius of that one only."""
    return np.concatenate([cluster(rng, c, 8) for c in _spots(n_vox)])


def before(pose, where):
    """The points that the pose moves to `where` (f64 arithmetic, rounded to float32): a source is laid out by where it lands."""
    cx, cy, cz = np.cos(pose[3:6])
    sx, sy, sz = np.sin(pose[3:6])
    R = (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
         @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))
    return ((np.asarray(where, np.float64) - np.asarray(pose[0:3])) @ R).astype(f32)


def row_source(rng, n_vox, n, pose):
    c = np.asarray(_spots(n_vox), np.float64)[rng.integers(0, n_vox, n)] + 0.5
    return before(pose, c + rng.uniform(-0.25, 0.25, (n, 3)))


def corner_target(rng):
    """Eight voxels whose points huddle at the corner the eight leaves share: every centroid is within the radius of every
    source point near that corner -- each (point, voxel) pair passes."""
    parts = []
    for k in (-1, 0):
        for j in (-1, 0):
            for i in (-1, 0):
                c = np.array([i, j, k], np.float64) * 0.3 + 0.15 + rng.uniform(-0.1, 0.1, (8, 3))
                parts.append(c.astype(f32))
    return np.concatenate(parts)


def pass_cases():
    out = []
    for n_vox, n, pose in [(1, 1, "general"), (63, 3, "general"), (63, 3, "snap_a"), (64, 511, "general"), (65, 512, "snap_b"),
                           (128, 513, "general"), (129, 513, "snap_a")]:
        rng = np.random.default_rng(100 + n_vox)
        out.append({"name": "v%d_n%d_%s" % (n_vox, n, pose), "tgt": row_target(rng, n_vox), "res": 1.0,
                    "src": row_source(rng, n_vox, n, POSES[pose]), "pose": POSES[pose], "expect": {"n": n, "n_vox": n_vox, "pairs": n}})
    rng = np.random.default_rng(200)
    corner = corner_target(rng)
    out.append({"name": "all_pass", "tgt": corner, "res": 1.0, "src": before(POSE_GENERAL, rng.uniform(-0.2, 0.2, (96, 3))),
                "pose": POSE_GENERAL, "expect": {"n": 96, "n_vox": 8, "pairs": 96 * 8}})
    out.append({"name": "none_pass", "tgt": corner, "res": 1.0, "src": before(POSE_GENERAL, rng.uniform(-0.2, 0.2, (70, 3)) + [5, 5, 5]),
                "pose": POSE_GENERAL, "expect": {"n": 70, "n_vox": 8, "pairs": 0}})
    rng = np.random.default_rng(201)
    tgt = np.concatenate([cluster(rng, (-6, -6, -4), 8), np.full((6, 3), 2.5, f32), cluster(rng, (-4, -6, -4), 8)])
    src = np.concatenate([row_source(rng, 2, 40, POSE_GENERAL), before(POSE_GENERAL, rng.uniform(-0.3, 0.3, (20, 3)) + 2.5)])
    out.append({"name": "zero_inverse", "tgt": tgt, "res": 1.0, "src": src, "pose": POSE_GENERAL, "expect": {"n": 60, "n_vox": 3}})
    rng = np.random.default_rng(203)
    src, bad = row_source(rng, 65, 130, POSE_GENERAL), [0, 63, 64, 65, 129]   # one record per workgroup (n < 512): every edge is one
    for q, i in enumerate(bad):
        src[i, q % 3] = (NAN, INF, -INF)[q % 3]
    out.append({"name": "staged_nonfinite", "tgt": row_target(rng, 65), "res": 1.0, "src": src, "pose": POSE_GENERAL, "bad": bad,
                "expect": {"n": 130, "n_vox": 65, "pairs": 125}})
    rng = np.random.default_rng(202)
    out.append({"name": "empty_source", "tgt": corner, "res": 1.0, "src": np.zeros((0, 3), f32), "pose": POSE_GENERAL,
                "expect": {"n": 0, "n_vox": 8, "pairs": 0}})
    return out


# ---- large sources: a small one repeated --------------------------------------------------------------------------------------
PASS_BLOCKS = 512   # workgroups of a derivative pass: per_block = ceil(n / 512) records each


def bad_at(n):
    """Where the non-finite records of a tiled source go: the wave edges of a 256-thread workgroup (63, 64, 255, 256), the
    edges of the pass's workgroups for THIS n (per_block - 1, per_block, per_block + 1, the second and the last workgroup's
    first record and the one before it) and the last index.  Record 0 stays finite: a read that is off by one record loses
    it, and the sums notice."""
    pb = -(-n // PASS_BLOCKS)
    last = (n - 1) // pb * pb
    at = {63, 64, 255, 256, pb - 1, pb, pb + 1, 2 * pb - 1, 2 * pb, last - 1, last, n - 1}
    return sorted(i for i in at if 0 < i < n)


def tiled_source(base, n, seed):
    """n records: the rows of `base` repeated in a shuffled order, records with one non-finite coordinate put at bad_at(n).
    Returns (src [n x 3], mult [len(base)]: how often each base row occurs, bad: the indices of the others)."""
    rng = np.random.default_rng(seed)
    bad = np.array(bad_at(n))
    good = n - len(bad)
    pick = np.concatenate([np.tile(np.arange(len(base)), good // len(base)), np.arange(good % len(base))])
    pick = pick[rng.permutation(good)]
    src = np.empty((n, 3), f32)
    mask = np.ones(n, bool)
    mask[bad] = False
    src[mask] = base[pick]
    src[bad] = base[0]
    for q, i in enumerate(bad):
        src[i, q % 3] = (NAN, INF, -INF)[q % 3]
    return src, np.bincount(pick, minlength=len(base)), bad


LARGE_N = [262144, 262145, 1000003]   # 512 workgroups: 512 points each (staged in LDS), 513 (read where they lie), 1954
