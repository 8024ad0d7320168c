"""The cases of tests/test_icp_scale_cpu.py and tests/test_icp_scale_gpu.py: targets, sources and gates of the ICP correspondence search
across the float32 range.  Built on tests/scale_cases.py (BASES, WINDOW, EXTREME, MIXED, scaled); no GPU is touched here, everything
is float32 from fixed seeds, 2 000 target and 1 500 source records a case at most.

A source is a permuted subset of the target's finite records, each moved by about 1 % of the extent (normal, sigma = 1 % of the
longest side of the box), made at scale 1 and then scaled with the target, so that scaled(source, e) goes with scaled(target, e).

  A  window    BASES x WINDOW: target, source and gate times 2^e.  Gates: 3 % of the extent (times 2^e), and unbounded.
  B  offsets   `uniform` and its source moved by 2^10, 2^17, 2^23 m along x and along all three axes, rounded to float32: records
               collapse into copies and ties.  Gates: 0.05 m and unbounded.
  C  outside   `uniform` and `copies` at the exponents of EXTREME (gates as in A), and every cloud of MIXED as the target, its source
               scale_cases.jittered records of its own (gates: the median nearest distance of the reference, and unbounded).
  D  far       a unit box of 2 000 records; queries 2^k m outside it, k = 5 .. 100, along three axes and two diagonals: 760 cells
               outside at k = 5, 1 520 at k = 6 -- either side of kFarCells = 1 024 (icp_kernels.hpp), beyond which a query takes no bound
               but every point.  Gates: 0.2 m (every query comes back -1) and unbounded (ties among floats: the lowest index wins).
               And once more with a gate of +inf (D-far-inf): beyond 2^64 m every d2 is +inf, +inf ties with +inf, record 0 wins and
               the pair is ACCEPTED (sqrt(DBL_MAX) rejects it).  Its sums are infinite: INF_GATE cases are searched, not summed.

The cost cap: a case goes to a GPU only if, for EVERY set of switches the suite builds its index with (TUNABLE_SETS: the default, the
forced brick hash, the small dense table), icp_grid_layout.cost_bound says that one search of one query touches at most 2^20
things and the case's searches (SEARCHES of every source record) at most 2^30.  OVER_CAP lists the cases that do not;
test_icp_scale_cpu.py asserts that the list is what the model says.  The limit behind it is stated at rsreg_icp_set_target
(include/rsreg.h); the rule is not changed.
The served range: over a target whose plan says served = False (a cell above 2^60 m, a box wider than a float: icp_grid_plan.hpp) every
search is refused (rsreg_icp_search, rsreg_icp_align); refused_ids() lists those cases, and the GPU test asserts the refusal.  No
search kernel runs for them.
GPU_FAMILIES: the families whose cases tests/test_icp_scale_gpu.py runs: all four.
"""
import collections
import functools
import math

import numpy as np

import icp_grid_layout as L
import icp_search_ref as R
import scale_cases as S

Case = collections.namedtuple("Case", "id family name e gate_kind far")

PER_QUERY_CAP = 1 << 20
PER_CASE_CAP = 1 << 30
SEARCHES = 11                      # test_icp_scale_gpu.py: search, search, and align() of one and of two iterations in three pipelines
TUNABLE_SETS = {"default": L.DEFAULT, "force_hash": L.DEFAULT._replace(dense_max_cells=0), "dense_2e6": L.DEFAULT._replace(dense_max_cells=2000000)}
OFFSETS = (10, 17, 23)
FAR_KS = tuple(range(5, 101))
FAR_DIRS = ((1, 0, 0), (0, -1, 0), (0, 0, 1), (1, 1, 1), (1, -1, 0))
C_BASES = ("uniform", "copies")
GPU_FAMILIES = ("A", "B", "C", "D")
INF_GATE = ("D-far-inf",)


def _cases():
    out = []
    for b in S.BASES:
        for e in S.WINDOW:
            for g in ("bounded", "unbounded"):
                out.append(Case("A-%s*2^%d-%s" % (b, e, g), "A", b, e, g, False))
    for k in OFFSETS:
        for axes in ("x", "xyz"):
            for g in ("bounded", "unbounded"):
                out.append(Case("B-2^%d-%s-%s" % (k, axes, g), "B", axes, k, g, True))
    for b in C_BASES:
        for e in S.EXTREME:
            for g in ("bounded", "unbounded"):
                out.append(Case("C-%s*2^%d-%s" % (b, e, g), "C", b, e, g, False))
    for m in S.MIXED:
        for g in ("bounded", "unbounded"):
            out.append(Case("C-%s-%s" % (m, g), "C", m, None, g, False))
    for g in ("bounded", "unbounded"):
        out.append(Case("D-far-%s" % g, "D", "unit_box", None, g, False))
    out.append(Case("D-far-inf", "D", "unit_box", None, "inf", False))
    return tuple(out)


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


def _frozen(a):
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


def _extent(xyz):
    mn, mx, _ = L.box_of(xyz)
    return float((mx.astype(np.float64) - mn.astype(np.float64)).max())


@functools.lru_cache(maxsize=None)
def base_source(name):
    """The source of a base cloud at scale 1 (float64, before any rounding): a permuted subset of its finite records, 1 500 at most,
    each moved by N(0, (1 % of the extent)^2) a coordinate."""
    xyz = S.base(name)
    rows = np.flatnonzero(R.finite_rows(xyz))
    rng = np.random.default_rng(4100 + S.BASES.index(name))
    rows = rng.permutation(rows)[:1500]
    return xyz[rows].astype(np.float64) + 0.01 * _extent(xyz) * rng.standard_normal((len(rows), 3))


@functools.lru_cache(maxsize=None)
def unit_box():
    return _frozen(np.random.default_rng(4200).random((2000, 3)))


@functools.lru_cache(maxsize=None)
def target(cid):
    c = BY_ID[cid]
    if c.family == "A" or (c.family == "C" and c.e is not None):
        return _frozen(S.scaled(S.base(c.name), c.e))
    if c.family == "B":
        off = np.ldexp(1.0, c.e) * (np.array([1.0, 0.0, 0.0]) if c.name == "x" else np.ones(3))
        return _frozen((S.base("uniform").astype(np.float64) + off).astype(np.float32))
    if c.family == "C":
        return S.mixed(c.name)
    return unit_box()


@functools.lru_cache(maxsize=None)
def source(cid):
    c = BY_ID[cid]
    if c.family == "A" or (c.family == "C" and c.e is not None):
        return _frozen(S.scaled(base_source(c.name).astype(np.float32), c.e))
    if c.family == "B":
        off = np.ldexp(1.0, c.e) * (np.array([1.0, 0.0, 0.0]) if c.name == "x" else np.ones(3))
        return _frozen((base_source("uniform") + off).astype(np.float32))
    if c.family == "C":
        tgt = S.mixed(c.name)
        rows = np.random.default_rng(4300 + S.MIXED.index(c.name)).permutation(len(tgt))[:1500]
        return _frozen(S.jittered(tgt[rows], seed=47))
    rows = []
    with np.errstate(over="ignore"):
        for k in FAR_KS:
            for d in FAR_DIRS:
                rows.append(0.5 + np.asarray(d, np.float64) * (0.5 + math.ldexp(1.0, k)))
    src = np.asarray(rows).astype(np.float32)
    assert np.isfinite(src).all()
    return _frozen(src)


@functools.lru_cache(maxsize=None)
def gate(cid):
    c = BY_ID[cid]
    if c.gate_kind == "unbounded":
        return R.UNBOUNDED
    if c.gate_kind == "inf":
        return math.inf
    if c.family == "A" or (c.family == "C" and c.e is not None):
        return math.ldexp(0.03 * _extent(S.base(c.name)), c.e)
    if c.family == "B":
        return 0.05
    if c.family == "D":
        return 0.2
    d2 = R.nearest(source(cid), target(cid))[1].astype(np.float64)
    ok = np.isfinite(d2) & (d2 > 0)
    return float(np.sqrt(np.median(d2[ok]))) if ok.any() else 1.0


@functools.lru_cache(maxsize=None)
def ref(cid):
    return R.search(source(cid), target(cid), gate(cid))


def ties(cid, chunk=128):
    """How many source records have two or more finite target records at their smallest d2."""
    s, t = source(cid), target(cid)
    tt = t[R.finite_rows(t)]
    n = 0
    for a in range(0, len(s), chunk):
        d2 = R.d2_f32(s[a:a + chunk][:, None, :], tt[None, :, :])
        n += int(((d2 == d2.min(axis=1)[:, None]).sum(axis=1) > 1).sum())
    return n


# ------------------------------------------------------------------------------------------------ plans and the cost cap
@functools.lru_cache(maxsize=None)
def plan(cid, tun_name="default"):
    return L.plan_of(target(cid), gate(cid), TUNABLE_SETS[tun_name])


def limit_of(cid):
    """The distance a search of this case can never look beyond: the gate, +inf for an unbounded one."""
    return gate(cid) if BY_ID[cid].gate_kind == "bounded" else math.inf


@functools.lru_cache(maxsize=None)
def cost(cid):
    """(touches of one search of one query, touches of the case), the largest over TUNABLE_SETS."""
    n_points = int(R.finite_rows(target(cid)).sum())
    per_query = max(L.cost_bound(plan(cid, t), limit_of(cid), n_points) for t in TUNABLE_SETS)
    return per_query, per_query * len(source(cid)) * SEARCHES


def under_cap(cid):
    q, c = cost(cid)
    return q <= PER_QUERY_CAP and c <= PER_CASE_CAP


# the cases the present rule puts above the cap (test_icp_scale_cpu.py: this IS what the model says): the unbounded gate of every
# cloud whose extent puts it on the extent / 60 000 branch -- a whole-grid search of 15 000 bricks or 60 000 rows a side
OVER_CAP = tuple(["A-%s*2^%d-unbounded" % (b, e) for b in S.BASES for e in (20, 40, 55)] +
                 ["C-%s*2^%d-unbounded" % (b, e) for b in C_BASES for e in (62, 66, 70, 100)] +
                 ["C-%s-unbounded" % m for m in ("one_at_1e30", "two_at_3e38", "wide_and_1e23")])


def served(cid):
    """Whether the case's target is searched at all (the same under every set of switches: asserted on the CPU)."""
    return plan(cid).served


def gpu_ids():
    """The cases tests/test_icp_scale_gpu.py searches, sums and aligns: GPU_FAMILIES, served, under the cap, with a gate that rejects +inf."""
    return [c.id for c in CASES if c.family in GPU_FAMILIES and c.id not in OVER_CAP and served(c.id) and c.id not in INF_GATE]


def refused_ids():
    """The cases over whose target every search is refused (no search kernel runs, so the cap does not bear on them)."""
    return [c.id for c in CASES if c.family in GPU_FAMILIES and not served(c.id)]
