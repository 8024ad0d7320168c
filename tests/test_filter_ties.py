"""The correspondence filters (reciprocal, trimmed rejector) on exact distance ties, copies of a point and both source
paths: sources of at most 65 536 points are searched in the caller's order, larger ones (and any with RSREG_SORT_SMALL=1)
merged into weighted distinct points in Morton order.  The spec breaks every tie by the lowest index: among equidistant
target points, among equidistant source points (reciprocal) and among equal distances at the trim's cut.

CPU: tests/filters_ref.py (cKDTree, float32 rescoring, ties closed exactly) against the brute-force restatement of
test_filters.py and against the oracle.  GPU: the engine against that reference record by record, then whole alignments
against the oracle."""
import contextlib
import functools
import os

import numpy as np
import pytest

import filters_ref as R
from test_filters import _np_filters

H = 2.0 ** -10                 # the lattice step: sums, squares and differences of its multiples are exact in float32
GATE = 0.01                    # 10.24 steps
# source offsets from a lattice point of the target (spacing 8 steps), in steps; every sign and axis order is used.
# Squared norms 0 .. 6, 8 and 16; (4, 0, 0) lies half way between two target points (the lower target index wins)
OFFSETS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 0, 0), (2, 1, 0), (2, 1, 1), (2, 2, 0), (4, 0, 0)]
AB_OFFSET = (2, 2, 1)          # squared norm 9: used by the two interleaved points at the cut alone


def _cloud(xyz):
    from rsreg_amd import POINT_DTYPE, PointCloud
    pts = np.zeros(len(xyz), POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["w"] = 1.0
    return PointCloud(pts, width=len(xyz), height=1, is_dense=False)


def _signed(rng, off, n):
    o = np.array(off, np.int64)[None, :].repeat(n, 0)
    o = np.take_along_axis(o, np.argsort(rng.random((n, 3)), 1), 1)
    return o * rng.choice([-1, 1], (n, 3))


@functools.lru_cache(maxsize=None)
def lattice_pair(n, seed=11):
    """(source, target, positions of the A copies, positions of the B copies) as (n, 3) float32.

    Target: n lattice points of spacing 8 steps around the origin, in shuffled index order.  Source: n records, each a
    random target point plus an offset of OFFSETS (so whole blocks of pairs have bit-equal d2, and several records can
    share a target point at the same distance), with records at (0, 0, 0) (a target point: d2 = 0), NaN and inf among
    them, and 12 copies of a point A interleaved in index order with 12 copies of a point B at the same distance from
    their targets, a distance no other record has."""
    rng = np.random.default_rng(seed + n)
    side = int(np.ceil((n / 2) ** (1 / 3)))
    g = np.stack(np.meshgrid(np.arange(-side, side), np.arange(-side, side), np.arange(-side // 2, side // 2 + 1), indexing="ij"), -1).reshape(-1, 3)
    g = g[np.argsort(np.abs(g).sum(1), kind="stable")][:n]           # the n lattice points nearest the origin (the origin among them)
    g = g[rng.permutation(n)] * 8
    tgt = (g * H).astype(np.float32)
    base = g[rng.integers(0, n, n)]
    kind = rng.integers(0, len(OFFSETS), n)
    off = np.zeros((n, 3), np.int64)
    for k, o in enumerate(OFFSETS):
        m = kind == k
        off[m] = _signed(rng, o, int(m.sum()))
    src = ((base + off) * H).astype(np.float32)
    src[rng.choice(n, n // 20, replace=False)] = 0.0                 # missing depth: identical records at the origin
    # A and B: one target point each, the same squared offset, copies at scattered indices interleaved in index order
    slots = np.sort(rng.choice(np.arange(1, n - 1), 24, replace=False))
    a_pos, b_pos = slots[0::2], slots[1::2]
    ta, tb = g[rng.integers(0, n)], g[rng.integers(0, n)]
    src[a_pos] = ((ta + np.array(AB_OFFSET)) * H).astype(np.float32)
    src[b_pos] = ((tb - np.array(AB_OFFSET)[::-1]) * H).astype(np.float32)
    bad = rng.choice(np.setdiff1d(np.arange(n), slots), 3 if n % 2 else 4, replace=False)   # (an even number of pairs)
    src[bad[0]] = np.nan
    src[bad[1], 1] = np.inf
    src[bad[2], 2] = -np.inf
    if len(bad) > 3:
        src[bad[3], 0] = np.nan
    return src, tgt, a_pos, b_pos


@functools.lru_cache(maxsize=None)
def quantized_frames(size):
    """(source, target) of the synthetic RealSense pair with xyz rounded to multiples of 2^-10 (depth in ~mm steps)."""
    from rsreg_amd import synth

    def q(c):
        p = R.xyz(c)
        return (np.round(p / H) * H).astype(np.float32)
    return q(synth.render_frame(1, size, "parity")), q(synth.render_frame(0, size, "parity"))


_REF = {}


def ref(src, tgt, reciprocal=0, ratio=0.0):
    """R.search with GATE, memoized per cloud (the clouds themselves are cached: 1 M points take seconds)."""
    key = (id(src), id(tgt), int(reciprocal), float(ratio))
    if key not in _REF:
        _REF[key] = R.search(src, tgt, GATE, reciprocal, ratio)
    return _REF[key]


def ratio_for_keep(keep, count):
    """A ratio whose trim keeps exactly `keep` of `count` pairs."""
    for f in (0.5, 0.25, 0.75):
        r = (keep + f) / count
        if R.trim_keep(r, count) == keep:
            return r
    raise AssertionError((keep, count))


def tied_cut(src, tgt, reciprocal, frac=0.6):
    """A ratio whose cut falls inside a block of equal distances, near `frac` of the pairs."""
    pre, d2, count = ref(src, tgt, reciprocal)
    cand = np.nonzero(pre >= 0)[0]
    sd = np.sort(d2[cand])
    ties = np.nonzero(sd[1:] == sd[:-1])[0] + 1                      # keep = p splits a tied block
    assert len(ties), "no tied block in this cloud"
    keep = int(ties[np.argmin(np.abs(ties - frac * count))])
    return ratio_for_keep(keep, count)


def ab_cut(src, tgt, a_pos, b_pos):
    """Trimmed alone: a ratio whose cut keeps the first 5 of the 24 interleaved A / B copies (both kinds on each side)."""
    pre, d2, count = ref(src, tgt)
    dab = d2[a_pos[0]]
    assert (d2[b_pos] == dab).all() and (d2[a_pos] == dab).all()
    assert ((d2 == dab) & (pre >= 0)).sum() == 24                   # nobody else at that distance
    below = int(((d2 < dab) & (pre >= 0)).sum())
    return ratio_for_keep(below + 5, count)


def assert_cut_inside(src, tgt, reciprocal, ratio):
    pre, d2, count = ref(src, tgt, reciprocal)
    before, after = R.cut_block(pre, d2, count, ratio, pre)
    assert before > 0 and after > 0, (before, after)


# ---------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("reciprocal,ratio", [(0, 0.0), (1, 0.0), (0, 0.6), (1, 0.45), (0, 0.999), (1, 0.01)])
@pytest.mark.parametrize("seed", [5, 6])
def test_reference_matches_brute_force(reciprocal, ratio, seed):
    rng = np.random.default_rng(seed)
    tgt = rng.random((700, 3)).astype(np.float32)
    src = (tgt[rng.integers(0, 700, 900)] + rng.normal(0, 0.02, (900, 3))).astype(np.float32)
    src[100:110] = src[100]
    ni, nd = _np_filters(src, tgt, 0.05, reciprocal, ratio)
    ri, rd, _ = R.search(src, tgt, 0.05, reciprocal, ratio)
    np.testing.assert_array_equal(ri, ni)
    np.testing.assert_array_equal(rd[ni >= 0], nd[ni >= 0])


def test_reference_matches_brute_force_on_a_lattice():
    """Small lattice: many equidistant target points (half-spacing offsets) and source points, closed by widening k."""
    src, tgt, _, _ = lattice_pair(3000)
    fin = np.isfinite(src).all(1)
    for reciprocal, ratio in [(0, 0.0), (1, 0.0), (0, tied_cut(src, tgt, 0)), (1, tied_cut(src, tgt, 1))]:
        ni, nd = _np_filters(np.where(fin[:, None], src, 1e6).astype(np.float32), tgt, GATE, reciprocal, ratio)
        ri, rd, _ = R.search(src, tgt, GATE, reciprocal, ratio)
        np.testing.assert_array_equal(ri, ni)
        np.testing.assert_array_equal(rd[ni >= 0], nd[ni >= 0])


def _oracle_search(orc, src, tgt, reciprocal, ratio, guess=None):
    o = orc.IcpOracle()
    o.set_target(tgt, dedup=True)
    o.set_source(src)
    p = orc.IcpParams.default()
    p.max_iterations, p.criteria_mode, p.max_correspondence_distance, p.num_threads = 5, 1, GATE, 8
    p.use_reciprocal, p.trim_overlap_ratio = reciprocal, ratio
    o.begin(guess, p)
    oi, od = o.search()
    return oi, od, o.sums()


MODES = ["reciprocal", "trim-at-tie", "both-at-tie"]


@pytest.mark.parametrize("case,mode", [("lattice-50k", m) for m in MODES + ["trim-ab-copies"]]
                         + [("frames-N300-quantized", m) for m in MODES])
def test_reference_matches_oracle_on_ties(orc, case, mode):
    src, tgt = lattice_pair(50000)[:2] if case == "lattice-50k" else quantized_frames("N300")
    reciprocal = int(mode in ("reciprocal", "both-at-tie"))
    if mode == "reciprocal":
        ratio = 0.0
    elif mode == "trim-ab-copies":
        ratio = ab_cut(src, tgt, *lattice_pair(50000)[2:])
    else:
        ratio = tied_cut(src, tgt, reciprocal)
        assert_cut_inside(src, tgt, reciprocal, ratio)
    ri, rd, count = R.search(src, tgt, GATE, reciprocal, ratio)
    oi, od, os_ = _oracle_search(orc, src, tgt, reciprocal, ratio)
    np.testing.assert_array_equal(oi, ri)
    np.testing.assert_array_equal(od[ri >= 0], rd[ri >= 0])
    np.testing.assert_allclose(R.sums(src, tgt, ri, rd), os_, rtol=1e-11, atol=1e-11)
    assert (ri >= 0).sum() > 1000
    if mode == "trim-ab-copies":
        a_pos, b_pos = lattice_pair(50000)[2:]
        # the cut keeps A, B, A, B, A of the copies in index order: it splits the copies of both points
        kept = np.sort(np.concatenate([a_pos[ri[a_pos] >= 0], b_pos[ri[b_pos] >= 0]]))
        np.testing.assert_array_equal(kept, np.sort(np.concatenate([a_pos, b_pos]))[:5])


def test_reference_sizes_its_largest_cloud_quickly():
    import time
    src, tgt = quantized_frames("N1M")
    t0 = time.perf_counter()
    ri, _, count = R.search(src, tgt, GATE, 1, 0.5)
    assert time.perf_counter() - t0 < 30
    assert 0 < (ri >= 0).sum() == R.trim_keep(0.5, count)


# ---------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def api(rs):
    from rsreg_amd import api as a, lib
    lib.build()
    if a.device_count() < 1:
        pytest.fail("no HIP device: the product has no CPU fallback")
    return a


@contextlib.contextmanager
def _context(api, env):
    """A fresh context with `env` set (tunables are read when a context is created); afterwards the environment is put
    back and published again by another new context."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    ctx = api.Context(0)
    try:
        yield ctx
    finally:
        ctx.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        api.Context(0).close()


# size -> (clouds, environment, whether the source is merged and put in Morton order)
GPU_CASES = {
    "lattice-50k-sort-small": (lambda: lattice_pair(50000), {"RSREG_SORT_SMALL": "1"}, True),
    "lattice-65536": (lambda: lattice_pair(65536), {}, False),
    "lattice-65537": (lambda: lattice_pair(65537), {}, True),
    "frames-N300-quantized": (lambda: quantized_frames("N300") + (None, None), {}, True),
    "frames-N1M-quantized": (lambda: quantized_frames("N1M") + (None, None), {}, True),
}


def _icp(api, ctx, src, tgt, reciprocal, ratio, pipeline=0):
    icp = api.IterativeClosestPoint(ctx)
    icp.params = api.icp_params(max_iterations=5, criteria_mode=1, max_correspondence_distance=GATE, pipeline_mode=pipeline)
    icp.setUseReciprocalCorrespondences(reciprocal)
    icp.setTrimmedRejectorOverlapRatio(ratio)
    icp.setInputSource(src)
    icp.setInputTarget(tgt)
    return icp


def _first_iteration(api, ctx, src, tgt, reciprocal, ratio, reordered):
    """The engine's first search and sums against the reference, record by record."""
    icp = _icp(api, ctx, _cloud(src), _cloud(tgt), reciprocal, ratio)
    icp.begin(None)
    gi, gd = icp.search()
    gs = icp.sums()
    distinct = icp.grid_info().n_source_distinct
    icp.end()
    # the path this case is about: copies merged into distinct points only on the reordered path
    assert (distinct < len(src)) == reordered, (distinct, len(src))
    ri, rd, _ = ref(src, tgt, reciprocal, ratio)
    pre = ref(src, tgt)[0]
    np.testing.assert_array_equal(gi, ri)
    np.testing.assert_array_equal(gd[pre >= 0], rd[pre >= 0])
    rs = R.sums(src, tgt, ri, rd)
    assert gs[0] == int(gs[0]) == rs[0] == (ri >= 0).sum()
    np.testing.assert_allclose(gs, rs, rtol=1e-11, atol=1e-11)
    return gi, gd, gs


def _alignments(api, ctx, orc, src, tgt, reciprocal, ratio):
    """Whole alignments in every pipeline mode and from device clouds, against the oracle's."""
    o = orc.IcpOracle()
    o.set_target(tgt, dedup=True)
    o.set_source(src)
    p = orc.IcpParams.default()
    p.max_iterations, p.criteria_mode, p.max_correspondence_distance, p.num_threads = 5, 1, GATE, 8
    p.use_reciprocal, p.trim_overlap_ratio = reciprocal, ratio
    r = o.align(None, p)
    s_cloud, t_cloud = _cloud(src), _cloud(tgt)
    runs = [(pipeline, s_cloud, t_cloud) for pipeline in (0, 1, 2)]
    runs.append((0, api.DeviceCloud(s_cloud, ctx), api.DeviceCloud(t_cloud, ctx)))
    for pipeline, s, t in runs:
        icp = _icp(api, ctx, s, t, reciprocal, ratio, pipeline)
        icp.align(None)
        what = (pipeline, type(s).__name__)
        assert (icp.result.iterations, icp.result.n_correspondences) == (r.iterations, r.n_correspondences), what
        assert np.linalg.norm(icp.getFinalTransformation() - r.T) < 1e-5, what


@pytest.mark.gpu
@pytest.mark.parametrize("case,mode", [(c, m) for c in GPU_CASES for m in MODES]
                         + [(c, "trim-ab-copies") for c in GPU_CASES if c.startswith("lattice")])
def test_gpu_filters_on_ties(api, orc, case, mode):
    make, env, reordered = GPU_CASES[case]
    src, tgt, a_pos, b_pos = make()
    reciprocal = int(mode in ("reciprocal", "both-at-tie"))
    if mode == "reciprocal":
        ratio = 0.0
    elif mode == "trim-ab-copies":
        ratio = ab_cut(src, tgt, a_pos, b_pos)
    else:
        ratio = tied_cut(src, tgt, reciprocal)
        assert_cut_inside(src, tgt, reciprocal, ratio)
    with _context(api, env) as ctx:
        _first_iteration(api, ctx, src, tgt, reciprocal, ratio, reordered)
        _alignments(api, ctx, orc, src, tgt, reciprocal, ratio)


def exact_ratio(count):
    """A ratio near 1/2 whose float product with `count` is exactly an integer (the keep PCL computes without rounding)."""
    for keep in range(count // 2, count):
        r = float(np.float32(keep / count))
        if np.float32(r) * np.float32(count) == np.float32(keep):
            return r
    raise AssertionError(count)


def _edge_ratios(src, tgt, reciprocal):
    _, _, count = ref(src, tgt, reciprocal)
    return {"keep-0": ratio_for_keep(0, count), "keep-1": ratio_for_keep(1, count),
            "keep-count-1": ratio_for_keep(count - 1, count), "exactly-integral": exact_ratio(count)}


@pytest.mark.gpu
@pytest.mark.parametrize("reciprocal", [0, 1])
@pytest.mark.parametrize("edge", ["keep-0", "keep-1", "keep-count-1", "exactly-integral"])
@pytest.mark.parametrize("case", ["lattice-65536", "lattice-65537"])
def test_gpu_trim_edges(api, case, edge, reciprocal):
    make, env, reordered = GPU_CASES[case]
    src, tgt, _, _ = make()
    ratio = _edge_ratios(src, tgt, reciprocal)[edge]
    _, _, count = ref(src, tgt, reciprocal)
    keep = {"keep-0": 0, "keep-1": 1, "keep-count-1": count - 1}.get(edge, R.trim_keep(ratio, count))
    assert R.trim_keep(ratio, count) == keep and 0 < ratio < 1
    with _context(api, env) as ctx:
        gi, _, _ = _first_iteration(api, ctx, src, tgt, reciprocal, ratio, reordered)
    assert (gi >= 0).sum() == keep


@pytest.mark.gpu
@pytest.mark.parametrize("reciprocal", [0, 1])
@pytest.mark.parametrize("case", ["lattice-65536", "lattice-65537"])
def test_gpu_trim_off_is_no_filter(api, case, reciprocal):
    """ratio <= 0 or >= 1: no trimmed rejector, bit for bit the search and sums without one."""
    make, env, reordered = GPU_CASES[case]
    src, tgt, _, _ = make()
    with _context(api, env) as ctx:
        base = _first_iteration(api, ctx, src, tgt, reciprocal, 0.0, reordered)
        for ratio in (-0.5, 1.0, 1.5):
            got = _first_iteration(api, ctx, src, tgt, reciprocal, ratio, reordered)
            for a, b in zip(got, base):
                np.testing.assert_array_equal(a, b)
