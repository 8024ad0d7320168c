"""The cases of the pose-from-correspondences tests (tests/test_sac_cpu.py, tests/test_sac_gpu.py): clouds, correspondence lists
with a known share of exact pairs of a known motion, transforms to score, pairs built AT the threshold, and the sizes at which the
kernels take another path.  TILE, CHUNK, MAX_GROUPS and the batches mirror csrc/sac_plan.hpp; tests/test_sac_cpu.py checks them
against the header itself (tests/cpp/sac_plan_rule.cpp).
"""
import functools

import numpy as np

CORR = np.dtype([("index_query", np.int32), ("index_match", np.int32), ("distance", np.float32)])

BLOCK, PAIRS_PER_LANE, TILE, CHUNK, MAX_GROUPS, FIRST_BATCH, MAX_BATCH, TRIES = 256, 2, 512, 64, 4096, 256, 4096, 16

# pair counts: one, the least a model needs, a wave +- 1, a pair tile +- 1, several tiles with a ragged end
PAIR_COUNTS = (1, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 5003)
# hypothesis counts: one, a chunk (the least slice) +- 1, many slices
HYP_COUNTS = (1, CHUNK - 1, CHUNK, CHUNK + 1, 4096)
# with one pair tile a slice is one chunk up to MAX_GROUPS chunks; one hypothesis more and a slice is two chunks: the last
# workgroup's second chunk holds that one hypothesis
HYP_SLICE_EDGE = (MAX_GROUPS * CHUNK - 1, MAX_GROUPS * CHUNK, MAX_GROUPS * CHUNK + 1, MAX_GROUPS * CHUNK + CHUNK + 1)


def plan(n, H):
    """(tiles, chunks, slice_chunks, slices) of csrc/sac_plan.hpp"""
    tiles, chunks = -(-n // TILE), -(-H // CHUNK)
    per = min(max(1, -(-(tiles * chunks) // MAX_GROUPS)), chunks)
    return tiles, chunks, per, -(-chunks // per)


def batch(done, max_iterations):
    if done >= max_iterations:
        return 0
    b, start = FIRST_BATCH, 0
    while start + b <= done:
        start += b
        b = min(2 * b, MAX_BATCH)
    return min(b, max_iterations - done)


def rigid(axis, angle, t):
    """4 x 4 float64: the rotation by `angle` about `axis`, then the translation t"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    M[:3, 3] = t
    return M


MOTION = rigid((0.3, -0.5, 0.8), 2.1, (0.7, -1.3, 0.4))   # 120 degrees and more than a cloud's half width: far outside ICP's basin


def records(xyz, stride=16, seed=0):
    """`stride`-byte records that start with x, y, z; random bits behind them"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rng = np.random.default_rng(1000 + seed)
    raw = rng.integers(0, 256, (len(xyz), stride), dtype=np.uint8)
    raw[:, :12] = xyz.view(np.uint8).reshape(len(xyz), 12)
    dt = np.dtype({"names": ["x", "y", "z"], "formats": ["<f4"] * 3, "offsets": [0, 4, 8], "itemsize": stride})
    return raw.view(dt).reshape(-1)


@functools.lru_cache(maxsize=None)
def motion_case(n=2000, share=0.4, seed=1):
    """(source xyz, target xyz, corr, true): n pairs over two clouds of n points in [-2, 2]^3.  `true` marks round(share * n) pairs
    whose target point is MOTION applied to the source point in float64, rounded to float32; the target point of every other pair
    is random.  The pairs come in a shuffled order and name shuffled records."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    tgt = rng.uniform(-3.5, 3.5, (n, 3)).astype(np.float32)
    true = np.zeros(n, bool)
    true[rng.permutation(n)[:int(round(share * n))]] = True
    qi, mi = rng.permutation(n), rng.permutation(n)
    moved = (src[qi].astype(np.float64) @ MOTION[:3, :3].T + MOTION[:3, 3]).astype(np.float32)
    tgt[mi[true]] = moved[true]
    corr = np.zeros(n, CORR)
    corr["index_query"], corr["index_match"], corr["distance"] = qi, mi, rng.uniform(0, 100, n).astype(np.float32)
    for a in (src, tgt, corr, true):
        a.setflags(write=False)
    return src, tgt, corr, true


def transforms(H, seed=0):
    """(H, 4, 4) float32: MOTION disturbed by a rotation of 0 .. 0.05 rad and a shift of 0 .. 0.1, so that the counts spread from
    every true pair down to a handful; every 7th is a random rigid motion"""
    rng = np.random.default_rng(77 + seed)
    out = np.zeros((H, 4, 4), np.float32)
    for h in range(H):
        if h % 7 == 6:
            out[h] = rigid(rng.normal(size=3), rng.uniform(0, np.pi), rng.uniform(-2, 2, 3))
        else:
            s = rng.uniform(0, 1) ** 2
            out[h] = rigid(rng.normal(size=3), 0.05 * s, rng.uniform(-0.1, 0.1, 3) * s) @ MOTION
    return out


def transforms_fast(H, seed=0):
    """transforms() for very many H: a few hundred distinct ones, repeated in a shuffled order"""
    base = transforms(331, seed)
    return base[np.random.default_rng(seed).integers(0, len(base), H)]


def threshold_pairs(threshold, seed=0, each=8):
    """(source xyz, target xyz, corr, d2): pairs whose float32 d2 under the IDENTITY is exactly f = (float)(threshold^2), its lower
    and its upper float neighbour -- `each` of each, found by search: p = 0 and q = s * u with u a random direction and s within a
    few ulps of sqrt(f); (dx * dx + dy * dy) + dz * dz is then evaluated as the contract does and the hits are kept."""
    f = np.float32(float(threshold) * float(threshold))
    want = [np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(np.inf))]
    rng = np.random.default_rng(5 + seed)
    u = rng.normal(size=(20000, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    q = (u * (np.sqrt(np.float64(f)) * (1 + rng.uniform(-3e-7, 3e-7, len(u)))[:, None])).astype(np.float32)
    d2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]).astype(np.float32) + q[:, 2] * q[:, 2]).astype(np.float32)
    pick = np.concatenate([np.flatnonzero(d2 == w)[:each] for w in want])
    assert len(pick) == 3 * each, "the search did not hit every neighbour of the threshold"
    tgt = q[pick]
    src = np.zeros_like(tgt)
    corr = np.zeros(len(pick), CORR)
    corr["index_query"] = corr["index_match"] = np.arange(len(pick))
    return src, tgt, corr, d2[pick]


def nonfinite_case(seed=3):
    """motion_case(300) with NaN, +inf and -inf put into source and target points that pairs name, true pairs among them"""
    src, tgt, corr, true = (a.copy() for a in motion_case(300, 0.5, seed))
    bad_s, bad_t = corr["index_query"][[5, 17, 40, 41]], corr["index_match"][[60, 61, 90, 17]]
    src[bad_s[0], 0], src[bad_s[1], 1], src[bad_s[2], 2], src[bad_s[3]] = np.nan, np.inf, -np.inf, np.nan
    tgt[bad_t[0], 2], tgt[bad_t[1], 0], tgt[bad_t[2]], tgt[bad_t[3], 1] = np.nan, np.inf, -np.inf, np.nan
    return src, tgt, corr, true


def repeated_sources_case(distinct=5, n=200, seed=4):
    """motion_case whose pairs name only `distinct` source records: most triples hold a source point twice and are drawn again"""
    src, tgt, corr, true = (a.copy() for a in motion_case(n, 0.6, seed))
    keep = corr["index_query"][:distinct]
    rng = np.random.default_rng(seed)
    corr["index_query"] = keep[rng.integers(0, distinct, n)]
    moved = (src[corr["index_query"]].astype(np.float64) @ MOTION[:3, :3].T + MOTION[:3, 3]).astype(np.float32)
    tgt[corr["index_match"][true]] = moved[true]
    return src, tgt, corr, true


def one_source_case(n=50, seed=6):
    """every pair names the SAME source record: no try is ever good, every hypothesis is invalid"""
    src, tgt, corr, true = (a.copy() for a in motion_case(n, 0.5, seed))
    corr["index_query"] = corr["index_query"][0]
    return src, tgt, corr, true


# the rejector's cases: name -> (case, parameters).  What each is FOR is asserted by tests/test_sac_cpu.py on the reference.
SAC_CASES = {
    "first_batch": (lambda: motion_case(2000, 0.4, 1), dict(seed=11)),
    "later_batch": (lambda: motion_case(2000, 0.2, 2), dict(seed=12, max_iterations=2000)),
    "to_max_iterations": (lambda: motion_case(2000, 0.2, 2), dict(seed=13, max_iterations=300)),
    "repeated_sources": (lambda: repeated_sources_case(), dict(seed=14, max_iterations=400)),
    "min_sample_distance": (lambda: motion_case(500, 0.5, 7), dict(seed=15, min_sample_distance=3.2, max_iterations=400)),
    "all_invalid": (lambda: one_source_case(), dict(seed=16)),
    "nonfinite": (lambda: nonfinite_case(), dict(seed=17, max_iterations=300)),
    "two_pairs": (lambda: tuple(a[:2] if i == 2 else a for i, a in enumerate(motion_case(300, 0.5, 3))), dict(seed=18)),
}
