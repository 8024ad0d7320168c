"""The clouds of tests/test_scale_cpu.py and tests/test_scale_gpu.py: the small clouds of tests/fpfh_cases.py moved across the float32
range, and clouds that mix magnitudes.  No GPU is touched here; everything is float32, from fixed seeds, 2 000 records at most.

Scaling by a power of two commutes with every float32 and float64 operation of the cloud searches as long as nothing overflows
or becomes a denormal, so inside that window the outputs at scale 2^e are the outputs at scale 1 moved by exact powers of two
(test_scale_cpu.py establishes the window on the references alone).  Outside it the float32 brute-force references are the oracle.

  WINDOW     exponents at which no output of any base cloud leaves the normal float32 range;
  EXTREME    exponents at which squared distances overflow (62 and up) or are denormals or zero (-62 and down);
  MIXED      clouds built from uniform() that mix magnitudes:
    one_at_1e30      one more record at x = 1e30: 4 001 x 2 x 2 cells, cell * cell = +inf in float32;
    two_at_3e38      two more records at x = +-3e38: (q - origin) overflows for the upper one, and every record of the box itself
                     sits at origin + 3e38 in float32;
    wide_and_1e23    the box at 2^66 (extent 1.5e20) and one more record at x = 1e23: the cell is 2.5e19, cell * cell = +inf, while the
                     records of the box are a few cells apart and their squared distances are finite floats;
    tiny_and_one     the box at 2^-70 and one more record at x = 1;
    denormal         the box moved to positive coordinates, at 2^-140: every coordinate a float32 denormal, every d2 zero.
  FAR_TARGETS  targets of a fitness score whose source also lies up to 1e32 cells outside the target's box (far_source).
"""
import collections
import functools

import numpy as np

import fitness_ref as F
import fpfh_cases
import normals_ref as N
import pointgrid_layout as G
import radius_ref as R
import sor_ref as S

WINDOW = (-40, -20, 20, 40, 55)
EXTREME = (-120, -70, -62, 62, 66, 70, 100)
BASES = ("uniform", "sphere", "plane", "copies", "holes")
MIXED = ("one_at_1e30", "two_at_3e38", "wide_and_1e23", "tiny_and_one", "denormal")
KS = (1, 10, 64)              # knn(k); knn_mean_distance(k) needs k + 1 columns
NORMAL_KS = (10, 50)
STD_MUL = 1.0                 # the SOR threshold of the keep mask
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)


def scaled(xyz, e):
    """xyz * 2^e, exactly where nothing overflows or becomes a denormal."""
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(np.asarray(xyz, np.float32), int(e)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def base(name):
    """(n, 3) float32, read-only: a cloud of fpfh_cases at scale 1."""
    if name == "uniform":
        xyz = fpfh_cases.uniform()
    elif name == "sphere":
        xyz = fpfh_cases.sphere()
    elif name == "plane":
        xyz = fpfh_cases.plane()
    elif name == "copies":
        xyz = fpfh_cases.copies()
    elif name == "holes":
        xyz = fpfh_cases.holes()[0]
    else:
        raise KeyError(name)
    xyz = np.ascontiguousarray(xyz, np.float32)
    assert len(xyz) <= 2000
    xyz.setflags(write=False)
    return xyz


def bad_normals(name):
    """The records of `holes` whose normal the FPFH tests make non-finite (fpfh_cases.holes), else none."""
    return fpfh_cases.holes()[1] if name == "holes" else np.zeros(0, np.int64)


@functools.lru_cache(maxsize=None)
def mixed(name):
    u = fpfh_cases.uniform()
    if name == "one_at_1e30":
        xyz = np.concatenate([u, [[1e30, u[0, 1], u[0, 2]]]])
    elif name == "two_at_3e38":
        xyz = np.concatenate([u, [[3e38, u[0, 1], u[0, 2]], [-3e38, u[1, 1], u[1, 2]]]])
    elif name == "wide_and_1e23":
        big = scaled(u, 66)
        xyz = np.concatenate([big, [[1e23, big[0, 1], big[0, 2]]]])
    elif name == "tiny_and_one":
        xyz = np.concatenate([scaled(u, -70), [[1.0, 0.0, 0.0]]])
    elif name == "denormal":
        xyz = scaled((u + np.float32([3.0, 2.0, 1.0])).astype(np.float32), -140)
        assert (xyz > 0).all() and (xyz < FLT_MIN).all()
    else:
        raise KeyError(name)
    xyz = np.ascontiguousarray(xyz, np.float32)
    assert np.isfinite(xyz).all() and len(xyz) <= 2000
    xyz.setflags(write=False)
    return xyz


def cloud_of(case):
    """case: (base name, exponent) or a MIXED name."""
    if isinstance(case, str):
        return mixed(case)
    return scaled(base(case[0]), case[1])


def label(case):
    return case if isinstance(case, str) else "%s*2^%d" % case


OUTSIDE = [(b, e) for b in BASES for e in EXTREME] + list(MIXED)


def jittered(xyz, seed=31):
    """A copy of the cloud with every coordinate moved by about a thousandth of itself: the source of a fitness score against the
    cloud.  Made at the cloud's own scale, so scaled(jittered(x), e) is the source that goes with scaled(x, e)."""
    rng = np.random.default_rng(seed)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(xyz, np.float64) * (1.0 + 1e-3 * rng.standard_normal(np.shape(xyz)))).astype(np.float32)


# targets of a fitness score whose source also holds records far outside the target's box
FAR_TARGETS = (("uniform", -70), ("uniform", -30), ("uniform", 0), ("uniform", 40))
FAR_CELLS = (1e3, 1e9, 1e15, 3e17, 3e18, 1e20, 1e25, 1e32)


@functools.lru_cache(maxsize=None)
def far_source(case):
    """The source of a fitness score against cloud_of(case): every tenth record of the jittered target, and records FAR_CELLS cells
    of the fitness grid beyond the box along +x, along -y and along the diagonal (those that are finite floats), and two at the
    ends of the float range."""
    tgt = cloud_of(case)
    lay = G.layout_of(tgt, "fit")
    mn, mx = tgt.min(axis=0).astype(np.float64), tgt.max(axis=0).astype(np.float64)
    mid = 0.5 * (mn + mx)
    rows = [p for p in jittered(tgt)[::10]]
    with np.errstate(over="ignore"):
        for cells in FAR_CELLS:
            d = cells * float(lay.cell)
            for p in ([mx[0] + d, mid[1], mid[2]], [mid[0], mn[1] - d, mid[2]], [mx[0] + d, mx[1] + d, mn[2] - d]):
                p = np.asarray(p).astype(np.float32)
                if np.isfinite(p).all():
                    rows.append(p)
    rows += [np.float32([3e38, 0.0, 0.0]), np.float32([-1e30, 1e30, 0.0])]
    src = np.asarray(rows, np.float32)
    src.setflags(write=False)
    return src


# ------------------------------------------------------------------------------------------------ the radii and ranges, at scale 1
def _just_above(r2):
    """A radius whose float32 square (float32 of the double r * r) is the float32 next above r2."""
    up = np.nextafter(np.float32(r2), np.float32(np.inf))
    r = float(np.sqrt(float(up)))
    while np.float32(r * r) < up:
        r = float(np.nextafter(r, np.inf))
    assert np.float32(r * r) == up
    return r


@functools.lru_cache(maxsize=None)
def radii(name):
    """The radii of a base cloud at scale 1, drawn from the reference: the median distance to the 32nd neighbour (a typical record has
    a few dozen neighbours); on `plane` the lattice spacing itself -- the four lattice neighbours lie AT the radius and are not
    counted -- and the radius whose float32 square is the next float above it, where they are."""
    xyz = base(name)
    fin = S.finite_rows(xyz)
    r = float(np.sqrt(np.median(brute(name, 0).d2[fin, 31].astype(np.float64))))
    if name == "plane":
        return (fpfh_cases.H, _just_above(fpfh_cases.H * fpfh_cases.H), r)
    return (r,)


def radius_at(r, e):
    return float(np.ldexp(r, int(e)))


@functools.lru_cache(maxsize=None)
def outside_radius(case):
    """A radius for an EXTREME or MIXED cloud: the median distance to the 32nd neighbour over the records where that is a finite
    float above 0, else the largest finite distance that occurs, else 1."""
    d2 = brute_of(case).d2
    col = d2[:, min(31, d2.shape[1] - 1)].astype(np.float64)
    ok = np.isfinite(col) & (col > 0)
    if ok.any():
        return float(np.sqrt(np.median(col[ok])))
    rest = d2[np.isfinite(d2) & (d2 > 0)]
    return float(np.sqrt(float(rest.max()))) if len(rest) else 1.0


def pass_limits(name):
    """(lo, hi) float32 of a PassThrough on z at scale 1: the quartiles of the finite records' z."""
    z = base(name)[S.finite_rows(base(name)), 2]
    lo, hi = np.float32(np.quantile(z, 0.25)), np.float32(np.quantile(z, 0.75))
    return lo, hi                                 # (plane: every z is 1, and so are both limits -- every record lies AT them, and stays)


@functools.lru_cache(maxsize=None)
def fitness_between(name):
    """The bounded max_range of a base cloud's fitness score at scale 1 (fitness_ranges)."""
    return fitness_ranges(jittered(base(name)), base(name))[1]


# ------------------------------------------------------------------------------------------------ references, computed once
Brute = collections.namedtuple("Brute", "idx d2")


def _brute(xyz):
    fin = int(S.finite_rows(xyz).sum())
    idx, d2 = N.knn(xyz, min(65, fin), method="brute")
    idx.setflags(write=False)
    d2.setflags(write=False)
    return Brute(idx, d2)


@functools.lru_cache(maxsize=None)
def brute(name, e):
    """normals_ref.knn of a base cloud at 2^e, brute force, at k = 65: its first k columns are the reference at k (ascending by
    (d2, index): a prefix of the order)."""
    return _brute(scaled(base(name), e))


@functools.lru_cache(maxsize=None)
def brute_of(case):
    return brute(*case) if not isinstance(case, str) else _brute(mixed(case))


def knn_ref(b, k):
    return b.idx[:, :k], b.d2[:, :k]


def mean_ref(xyz, b, mean_k):
    """sor_ref.knn_mean_distance from the brute force's mean_k + 1 smallest d2, by sor_ref's own sum."""
    fin = S.finite_rows(xyz)
    out = np.zeros(len(xyz), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        out[fin] = S._mean_of_sorted(b.d2[fin][:, :mean_k + 1], mean_k)
    return out


def counts_brute(xyz, radius):
    """radius_ref's definition by a plain float32 brute force: d2 < r2_f32(radius), strictly, the record itself included; 0 for a
    non-finite record.  (radius_ref.search takes its candidates from a float64 tree with a relative margin, which is not argued for
    squared distances in the float32 denormals; test_scale_cpu.py holds the two against each other where it is.)"""
    xyz = np.asarray(xyz, np.float32)
    fin = np.flatnonzero(S.finite_rows(xyz))
    t = xyz[fin]
    out = np.zeros(len(xyz), np.uint32)
    r2 = R.r2_f32(radius)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for s in range(0, len(t), 256):
            out[fin[s:s + 256]] = (F.d2_f32(t[s:s + 256, None, :], t[None, :, :]) < r2).sum(axis=1)
    return out


def fitness_ranges(src, tgt):
    """(DBL_MAX, a range between two nearest squared distances that occur -- None where fewer than two finite ones do)."""
    d = F.nearest_d2_brute(src, tgt)
    occ = np.unique(d[np.isfinite(d)].astype(np.float64))
    between = 0.5 * (occ[len(occ) // 2 - 1] + occ[len(occ) // 2]) if len(occ) >= 2 else None
    return F.DBL_MAX, between


# ------------------------------------------------------------------------------------------------ the regime of a layout
Regime = collections.namedtuple("Regime", "cell_finite cell2 q_minus_origin d2 dims branch cell")


def _class(v):
    v = np.float32(v)
    if not np.isfinite(v):
        return "inf"
    if v == 0:
        return "0"
    return "denormal" if abs(float(v)) < FLT_MIN else "finite"


def regime(xyz, policy="knn", b=None):
    """What the point grid's float32 arithmetic does on this cloud: whether the cell is finite; what cell * cell is in float32
    ("finite", "inf", "0" or "denormal"); whether float32(q - origin) stays finite for every record ("finite" / "overflows"); and
    which kinds of squared distance occur among every record's 65 nearest: "normal", "denormal", "inf", and "underflow" (0 between
    two records that are not copies of each other)."""
    xyz = np.asarray(xyz, np.float32)
    lay = G.layout_of(xyz, policy)
    ok = S.finite_rows(xyz)
    with np.errstate(over="ignore", under="ignore"):
        cell2 = np.float32(lay.cell) * np.float32(lay.cell)
        rel = (xyz[ok] - lay.origin).astype(np.float32)
    b = b if b is not None else _brute(xyz)
    d2, idx = b.d2[ok], b.idx[ok]
    kinds = set()
    if ((d2 >= FLT_MIN) & np.isfinite(d2)).any():
        kinds.add("normal")
    if ((d2 > 0) & (d2 < FLT_MIN)).any():
        kinds.add("denormal")
    if np.isinf(d2).any():
        kinds.add("inf")
    if ((d2 == 0) & (xyz[idx] != xyz[ok][:, None, :]).any(axis=2)).any():
        kinds.add("underflow")
    return Regime(bool(np.isfinite(lay.cell)), _class(cell2), "finite" if np.isfinite(rel).all() else "overflows",
                  tuple(sorted(kinds)), tuple(lay.dims), lay.branch, float(lay.cell))
