"""Inputs of the feature-matching tests (tests/test_feature_match_cpu.py, tests/test_feature_match_gpu.py): descriptor rows, (n, 33)
float32, generated from fixed seeds -- the smallest shapes at which the search can still go wrong, a few thousand rows at most.

TILE, QUERIES, FILL, plan() and slice_begin() restate csrc/feature_plan.hpp; tests/test_feature_match_cpu.py holds them against the
header itself (tests/cpp/feature_plan_rule.cpp), so the cases know where a tile and a slice begin without a switch in the library.
There is no case past a launch cap: the search's grid is one uncapped launch dimension (the rule's table goes to 2^31 - 17 rows), so
the kernels have no grid-stride loop to cross.
"""
import functools

import numpy as np

DIM = 33
TILE, QUERIES, FILL = 64, 64, 2048
KS = (1, 2, 5, 16)
KS_EDGE = (3, 4, 8, 9)        # the compile-time lists are 1, 2, 4, 8, 16: the first and the last k of the lists KS leaves out
NS = (1, 63, 64, 65, 1000)
EVERY_K_SIZES = ((65, 2500), (1000, 65))   # several slices and a second query block of one live lane; one slice, a full and a one-row tile


def nts(k):
    return (k, TILE - 1, TILE, TILE + 1, 2500)


def plan(nq, nt):
    """(query blocks, target slices) of csrc/feature_plan.hpp"""
    qblocks = -(-nq // QUERIES)
    want = -(-FILL // qblocks)
    most = max(1, nt // TILE)
    return qblocks, max(1, min(want, most))


def slice_begin(s, slices, nt):
    return s * nt // slices


# (ns, nt) the rule is tabulated on: every size of the tests, the corners of the rule, and sizes of real use
PLAN_TABLE = sorted({(ns, nt) for ns in NS for k in KS + KS_EDGE for nt in nts(k)} | set(EVERY_K_SIZES) |
                    {(1, 20000), (3000, 16), (65, 2500), (1, 1), (1, 127), (1, 128), (64, 64 * 2048), (64, 64 * 2048 + 63), (65, 64 * 2048), (2048 * 64, 5000),
                     (2048 * 64 + 1, 5000), (5000, 5000), (30000, 30000), (100000, 100000), (307200, 307200), (2 ** 31 - 17, 2 ** 31 - 17), (1, 2 ** 31 - 17)})


def exact_rows(n, seed):
    """Multiples of 0.25 in [0, 32], four levels: every diff^2 and every partial sum of a pair is a multiple of 2^-4 below 2^20 of
    them (33 * 128^2 = 540 672), exact in float32 -- ANY summation order gives the same d2, and equal d2 are everywhere."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.float32([0.0, 0.25, 0.5, 32.0]), size=(n, DIM), p=[0.49, 0.3, 0.19, 0.02]).astype(np.float32)


def order_rows(n, seed):
    """Magnitudes spread over 2^-20 .. 2^6: another summation order (pairwise, reversed, fused) changes bits of d2."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, DIM)) * 2.0 ** rng.integers(-20, 7, (n, DIM))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def exact():
    return _frozen(exact_rows(NS[-1], 101), exact_rows(2500, 102))


@functools.lru_cache(maxsize=None)
def order():
    return _frozen(order_rows(NS[-1], 103), order_rows(2500, 104))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _rigid():
    a = np.deg2rad(25.0)
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K, np.array([0.3, -0.2, 0.1])


@functools.lru_cache(maxsize=None)
def real():
    """(source rows, target rows): FPFH rows (k = 10) by tests/fpfh_ref.py over the normals of tests/normals_ref.py, no GPU.  Target:
    fpfh_cases.corner and the plane lattice, whose records away from its rim all share one row -- repeated rows, zero blocks,
    genuine ties.  Source: the corner sampled again and the lattice, both moved rigidly, and the first 100 target rows verbatim
    (matches at d2 = 0)."""
    import fpfh_cases as K
    import fpfh_ref as F
    import normals_ref as N

    def rows(xyz):
        xyz = np.ascontiguousarray(xyz, np.float32)
        return F.fpfh(xyz, np.ascontiguousarray(N.normals(xyz, 10).normal), 10).fpfh
    R, t = _rigid()
    tgt = np.concatenate([rows(K.corner()), rows(K.plane())])
    src = np.concatenate([rows(K.corner(1500, 31) @ R.T + t), rows(K.plane() @ R.T + t), tgt[:100]])
    return _frozen(src.astype(np.float32), tgt.astype(np.float32))


def copies(ns, nt, seed):
    """(source, target, planted): equal rows planted in the target at index 0, TILE - 1, TILE and at the first and the last row of
    every slice the host rule cuts at this size -- equal-d2 candidates in different tiles AND different slices.  Source row 0 IS the
    planted row (d2 = 0 to every copy); the middle source row is the planted row with one bin moved (one positive d2 to every
    copy)."""
    src, tgt = order_rows(ns, seed), order_rows(nt, seed + 1)
    hot = order_rows(1, seed + 2)[0]
    _, slices = plan(ns, nt)
    planted = {0, TILE - 1, TILE}
    for s in range(slices):
        planted |= {slice_begin(s, slices, nt), slice_begin(s + 1, slices, nt) - 1}
    planted = np.array(sorted(p for p in planted if 0 <= p < nt))
    tgt[planted] = hot
    src[0] = hot
    src[ns // 2] = hot
    if ns > 1:
        src[ns // 2, 7] += np.float32(0.375)
    return src, tgt, planted


COPIES_SIZES = ((1, 20000), (65, 2500), (3000, 16), (64, 200))


def holes(seed=105):
    """(source, target): NaN, +inf and -inf in the first or the last bin of some source and some target rows."""
    src, tgt = order_rows(300, seed), order_rows(400, seed + 1)
    rng = np.random.default_rng(seed + 2)
    for rows in (src, tgt):
        bad = rng.choice(len(rows), 36, replace=False)
        for n, (value, col) in enumerate((v, c) for v in (np.nan, np.inf, -np.inf) for c in (0, DIM - 1)):
            rows[bad[6 * n:6 * n + 6], col] = value
    src[0, 0] = np.nan                                    # the first and the last row among them
    tgt[-1, DIM - 1] = -np.inf
    return src, tgt


def few_valid(n_valid, nt=70, seed=106):
    """A target of nt rows of which exactly n_valid are valid, spread over two tiles."""
    tgt = order_rows(nt, seed)
    keep = np.random.default_rng(seed + 1).choice(nt, n_valid, replace=False)
    bad = np.setdiff1d(np.arange(nt), keep)
    tgt[bad[::2], 0] = np.nan
    tgt[bad[1::2], DIM - 1] = np.inf
    return tgt


BIG = np.float32(3e38)
OVERFLOW_BIN = 11
OVERFLOW_PLUS_TARGETS = 5     # target rows that share the source's +3e38: fewer than 16, so a 16th answer lies at +inf


@functools.lru_cache(maxsize=None)
def overflow(ns=130, nt=200, seed=107):
    """(source, target): every way a d2 becomes +inf, all rows finite floats.
      * every fourth source row times -2^120, every third target row times 2^120: a square overflows.  Such a source row is at +inf
        from EVERY target row: its k nearest are the k lowest valid target indices, against a list that starts empty;
      * bin OVERFLOW_BIN holds +3e38 in source rows 1, 9, 17, .. and -3e38 in target rows 1, 8, 15, ..: the difference itself
        overflows (3e38 - -3e38).  OVERFLOW_PLUS_TARGETS target rows hold +3e38 there instead: the only rows at a finite distance
        from those source rows, so their nearest is finite and their 16th is +inf;
      * the last source row is 1e19 in every bin: every square is finite and the SUM overflows at the fourth bin; the one before
        is 1e15 in every bin: far from every target row, at a finite distance from the ones that are not scaled."""
    src, tgt = order_rows(ns, seed), order_rows(nt, seed + 1)
    with np.errstate(over="ignore"):
        tgt[::3] = np.ldexp(tgt[::3], 120)
        src[::4] = -np.ldexp(src[::4], 120)
    src[1::8, OVERFLOW_BIN] = BIG
    tgt[1::7, OVERFLOW_BIN] = -BIG
    plus = np.arange(2, nt, 3)[-OVERFLOW_PLUS_TARGETS:]       # (not scaled, not among the -3e38 rows)
    plus = plus[(plus % 7) != 1]
    tgt[plus, OVERFLOW_BIN] = BIG
    src[-1] = np.float32(1e19)
    src[-2] = np.float32(1e15)
    assert np.isfinite(src).all() and np.isfinite(tgt).all()
    return _frozen(src, tgt)


@functools.lru_cache(maxsize=None)
def denormal(name):
    """(source, target) whose squared distances are float32 denormals while every input is a normal float: the key of the search is
    the float's bit pattern, so the answer is right only if no subtraction, product or sum of a pair flushes a denormal.
      "order"  order_rows * 2^-70: most d2 are denormal, none is zero, the last bits depend on the summation order;
      "exact"  exact_rows * 2^-73: every d2 is a denormal of a few bits (a difference of 0.25 squares to 2^-150, half of the
               smallest denormal: it rounds to 0), a few hundred distinct values, ties everywhere;
      "zeros"  rows of +0.0 and -0.0 alone: every d2 has the bits of +0, the lowest index wins."""
    if name == "order":
        src, tgt = np.ldexp(order_rows(200, 108), -70), np.ldexp(order_rows(300, 109), -70)
    elif name == "exact":
        src, tgt = exact_rows(200, 110), exact_rows(300, 111)
        near = (np.abs(src[:, None, :] - tgt[None, :, :]) <= 0.25).all(axis=2).any(axis=0)
        src, tgt = np.ldexp(src, -73), np.ldexp(tgt[~near], -73)          # (a target row 0.25 or less from a source row in every bin: d2 = 0, left out)
    elif name == "zeros":
        rng = np.random.default_rng(112)
        src, tgt = (np.where(rng.random((n, DIM)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32) for n in (70, 130))
    else:
        raise KeyError(name)
    assert src.dtype == np.float32 and tgt.dtype == np.float32
    return _frozen(src, tgt)


DENORMALS = ("order", "exact", "zeros")
FLT_MIN = np.finfo(np.float32).tiny


def self_rows():
    """The rows of the `source == target` tests: the real case's target -- repeated rows everywhere -- with three rows made invalid."""
    rows = real()[1].copy()
    rows[[5, 1000, 2899], [0, 32, 7]] = [np.nan, np.inf, -np.inf]
    return rows


def records(rows, stride=132, seed=0):
    """The rows as records of `stride` bytes (a void array): the 33 floats first, random BITS behind them."""
    rows = np.ascontiguousarray(rows, np.float32)
    raw = np.random.default_rng(1000 + seed).integers(0, 256, (len(rows), stride), dtype=np.uint8)
    raw[:, :DIM * 4] = rows.view(np.uint8).reshape(len(rows), DIM * 4)
    return np.ascontiguousarray(raw).view(np.dtype((np.void, stride))).reshape(-1)
