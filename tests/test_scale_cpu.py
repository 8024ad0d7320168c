"""The window in which scaling a cloud by 2^e commutes with the cloud searches, established on the references alone, and what the
point grid's float32 arithmetic does outside it (tests/scale_cases.py holds the clouds; tests/test_scale_gpu.py asks the kernels).

  * Reference invariance: for every base cloud and every e of WINDOW, every reference output that the GPU test compares is the
    output at scale 1 moved by the exact power of two -- normals_ref.knn (indices equal, d2 * 2^2e), sor_ref's mean distances
    (* 2^e) and keep mask, the radius counts (radius_ref.counts and the plain brute force of scale_cases, at r * 2^e) and
    radius_ref.normals, normals_ref.normals (dimensionless: the same bytes), fitness_ref.fitness (the count, score * 2^2e, with
    max_range * 2^2e), fpfh_ref.fpfh with the scale-1 normals (SPFH and FPFH: the same bytes) and sor_ref.passthrough_keep.
    So an assertion of the GPU test is never conditional on the code under test.  No exponent of WINDOW had to be replaced.
  * Layout invariance: pointgrid_layout.layout picks the same rule and the same cells per axis at every e of WINDOW, and the cell
    times exactly 2^e, under all three policies.  For every EXTREME exponent and every MIXED cloud the regime is printed and
    asserted: the cell is always finite (grid_layout never reaches an infinite cell: the floor emax / 4000 and the bisection keep
    it below the extent), cell * cell in float32 is finite, +inf, 0 or a denormal, float32(q - origin) stays finite or not, and
    which kinds of squared distance occur.  Among them at least one case each reaches cell^2 = inf, cell^2 = 0, an overflowing
    q - origin and denormal d2.  tests/cpp/grid_layout.cpp agrees on all of these boxes.
  * The bound the searches prune with (pointgrid_layout.grid_lb2, the kernels' arithmetic restated) stays below every float32
    distance on every EXTREME scale of `uniform` and every MIXED cloud, where the float32 product cell * cell is +inf, 0 or a
    denormal of a few bits (the bound is multiplied by the cell twice, and 4 * 2^-149 comes off); and for the sources of a fitness
    score that lie up to 1e32 cells outside a target box of any size (FAR_TARGETS: beyond kPosMax cells the position is a NaN).
  * The box of cells and the rows a radius search visits hold every neighbour on the same clouds, the record itself included
    where its position has overflowed (its box is then the whole axis).
  * The FPFH contract outside the window, on `uniform` (FPFH_REGIME): all d2 zero or all +inf give all-zero rows; a denormal d2 gives
    w = +inf and a row of NaNs in a finite record, which nan_rows does not name and is_dense has to.
  * The share of records the normals check leaves out (gap_ratio < 1e-3) is at most 5 % of uniform and sphere at scale 1, on the
    reference; inside the window it is the same share by invariance.
"""
import numpy as np
import pytest

import fitness_ref as F
import fpfh_cases
import fpfh_ref
import normals_ref as N
import pointgrid_layout as G
import radius_ref as R
import scale_cases as C
import sor_ref as S
from test_pointgrid_layout_cpu import _bounds, _same, program  # noqa: F401  (program: the fixture that compiles grid_layout.cpp)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _ldexp32(a, e):
    return np.ldexp(np.asarray(a, np.float32), int(e)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ reference invariance
@pytest.mark.parametrize("name", C.BASES)
def test_references_commute_with_powers_of_two(name):
    x0 = C.base(name)
    fin = S.finite_rows(x0)
    b0 = C.brute(name, 0)
    nrm = fpfh_cases.ref_normals(name) if name != "holes" else np.ascontiguousarray(N.normals(x0, 10).normal)
    nrm = nrm.copy()
    bad = C.bad_normals(name)
    nrm[bad[:20]] = np.nan
    nrm[bad[20:], 2] = np.inf
    normals0 = {k: N.normals(x0, k, knn_result=C.knn_ref(b0, k)) for k in C.NORMAL_KS}
    fp0 = fpfh_ref.fpfh(x0, nrm, 10, knn_result=C.knn_ref(b0, 10))
    src0 = C.jittered(x0)
    between = C.fitness_between(name)
    fit0 = {r: F.fitness(src0, x0, r, valid=F.finite_rows(src0)) for r in (F.DBL_MAX, between)}
    lo0, hi0 = C.pass_limits(name)
    keep0 = S.passthrough_keep(x0, 2, lo0, hi0)
    assert keep0.all() and lo0 == hi0 if name == "plane" else 0 < keep0.sum() < fin.sum()
    rad0 = {r: (C.counts_brute(x0, r), R.normals(x0, r)) for r in C.radii(name)}
    for r, (cnt, _) in rad0.items():
        np.testing.assert_array_equal(cnt, R.counts(x0, r))
    typical = np.median(rad0[C.radii(name)[-1]][0][fin])
    print("%s: %d records, radii %s, a typical record has %d neighbours within the last" % (name, len(x0), C.radii(name), typical))
    assert 20 <= typical <= 60
    if name == "plane":                                       # AT the spacing the four lattice neighbours are not counted; one ulp above they are
        at, above = rad0[C.radii(name)[0]][0], rad0[C.radii(name)[1]][0]
        assert at.max() == 1 and above.max() == 5 and above.min() == 3
    for e in C.WINDOW:
        xe = C.scaled(x0, e)
        be = C.brute(name, e)
        assert _bits(be.idx) == _bits(b0.idx), (name, e)
        assert _bits(be.d2) == _bits(_ldexp32(b0.d2, 2 * e)), (name, e)
        assert np.isfinite(be.d2).all() and ((be.d2 == 0) | (be.d2 >= C.FLT_MIN)).all()
        for k in C.KS:
            m0, me = C.mean_ref(x0, b0, k), C.mean_ref(xe, be, k)
            assert _bits(me) == _bits(_ldexp32(m0, e)), (name, e, k)
            if k == 10:
                np.testing.assert_array_equal(me, S.knn_mean_distance(xe, k, method="brute"))
                t0, te = S.sor_stats(x0, m0, C.STD_MUL)[3], S.sor_stats(xe, me, C.STD_MUL)[3]
                assert te == np.ldexp(t0, e)
                k0, ke = S.sor_keep(x0, m0, t0), S.sor_keep(xe, me, te)
                assert (k0 == ke).all() and 0 < (~ke).sum() < len(ke)
        for k in C.NORMAL_KS:
            ne = N.normals(xe, k, knn_result=C.knn_ref(be, k))
            assert _bits(ne.normal) == _bits(normals0[k].normal) and _bits(ne.curvature) == _bits(normals0[k].curvature), (name, e, k)
        for r, (cnt, nr0) in rad0.items():
            re_ = C.radius_at(r, e)
            assert R.r2_f32(re_) == _ldexp32(R.r2_f32(r), 2 * e)
            np.testing.assert_array_equal(C.counts_brute(xe, re_), cnt)
            np.testing.assert_array_equal(R.counts(xe, re_), cnt)
            nre = R.normals(xe, re_)
            assert _bits(nre.normal) == _bits(nr0.normal) and _bits(nre.curvature) == _bits(nr0.curvature), (name, e, r)
        srce = C.scaled(src0, e)
        for r, (score, count) in fit0.items():
            re_ = r if r == F.DBL_MAX else float(np.ldexp(r, 2 * e))
            got = F.fitness(srce, xe, re_, valid=F.finite_rows(srce))
            assert got[1] == count and got[0] == float(np.ldexp(score, 2 * e)), (name, e, r, got, (score, count))
        assert 0 < fit0[between][1] < fit0[F.DBL_MAX][1]
        fpe = fpfh_ref.fpfh(xe, nrm, 10, knn_result=C.knn_ref(be, 10))
        assert _bits(fpe.spfh) == _bits(fp0.spfh) and _bits(fpe.fpfh) == _bits(fp0.fpfh), (name, e)
        assert (fpe.fragile_nb == fp0.fragile_nb).all() and (fpe.nan_rows == fp0.nan_rows).all()
        assert (S.passthrough_keep(xe, 2, _ldexp32(lo0, e), _ldexp32(hi0, e)) == keep0).all()


# ------------------------------------------------------------------------------------------------ layout invariance, and the regimes
def _rows(xyz, radius):
    mn, mx, nfin = G.box_of(xyz)
    return [(tuple(mn), tuple(mx), nfin, 0.0, "knn"), (tuple(mn), tuple(mx), nfin, 0.0, "fit"), (tuple(mn), tuple(mx), nfin, float(radius), "radius")]


@pytest.mark.parametrize("name", C.BASES)
def test_layout_commutes_with_powers_of_two(program, name):
    r = C.radii(name)[-1]
    lay0 = _same(program, _rows(C.base(name), r))
    for e in C.WINDOW:
        laye = _same(program, _rows(C.scaled(C.base(name), e), C.radius_at(r, e)))
        for a, b in zip(lay0, laye):
            assert (b.branch, b.dims, b.capped) == (a.branch, a.dims, a.capped), (name, e, a, b)
            assert b.cell == np.ldexp(a.cell, e) and np.isfinite(b.cell), (name, e, a, b)


# what every EXTREME exponent does to every base cloud, and every MIXED cloud: (cell * cell in float32, float32(q - origin))
CELL2 = {-120: "0", -70: "0", -62: "denormal", 62: "finite", 66: "finite", 100: "inf"}      # (70: inf or finite, by the cloud's extent)
MIXED_REGIME = {"one_at_1e30": ("inf", "finite"), "two_at_3e38": ("inf", "overflows"), "wide_and_1e23": ("inf", "finite"),
                "tiny_and_one": ("finite", "finite"), "denormal": ("0", "finite")}


def test_regimes_outside_the_window(program):
    seen = []
    for case in C.OUTSIDE:
        xyz = C.cloud_of(case)
        reg = C.regime(xyz, "knn", C.brute_of(case))
        print("%-16s cell %.6g (%s), %d x %d x %d; cell^2 in float32: %s; float32(q - origin): %s; d2 among the 65 nearest: %s" %
              (C.label(case), reg.cell, reg.branch, *reg.dims, reg.cell2, reg.q_minus_origin, ", ".join(reg.d2)))
        lays = _same(program, _rows(xyz, C.outside_radius(case)) + _rows(xyz, 1e30)[2:])
        assert all(np.isfinite(l.cell) and l.cell > 0 and l.inv_cell > 0 and max(l.dims) <= G.GRID_MAX_AXIS for l in lays), (case, lays)
        assert reg.cell_finite
        if isinstance(case, str):
            assert (reg.cell2, reg.q_minus_origin) == MIXED_REGIME[case], (case, reg)
        else:
            assert reg.q_minus_origin == "finite"
            assert reg.cell2 == CELL2[case[1]] if case[1] != 70 else reg.cell2 in ("inf", "finite"), (case, reg)
            if case[1] <= -100:
                assert reg.d2 == ("underflow",)
            if case[1] in (-62, -70):
                assert "denormal" in reg.d2
            if case[1] >= 70:                                  # (66: by the cloud's extent)
                assert "inf" in reg.d2
            if case[1] == 62:
                assert reg.d2 == ("normal",)
        seen.append(reg)
    assert any(r.cell2 == "inf" and "normal" in r.d2 for r in seen)         # the bound's product overflows before the distances do
    assert any(r.cell2 == "0" and "denormal" in r.d2 for r in seen)         # ... and underflows while they still tell records apart
    assert any(r.cell2 == "denormal" for r in seen)
    assert any(r.q_minus_origin == "overflows" for r in seen)
    assert any("denormal" in r.d2 for r in seen)
    reg = C.regime(C.mixed("denormal"))
    assert reg.d2 == ("underflow",) and reg.dims == (2, 2, 2) and reg.branch == "1e-30"


@pytest.mark.parametrize("case", [("uniform", e) for e in C.EXTREME] + list(C.MIXED), ids=C.label)
def test_bound_stays_below_every_float_distance(case):
    xyz = C.cloud_of(case)
    for policy in ("knn", "fit"):
        lay = G.layout_of(xyz, policy)
        queries = None if policy == "knn" else np.concatenate([C.jittered(xyz)[::3], xyz[::7]])
        cell_ratio, face_ratio, holds = _bounds(xyz, lay, queries)
        print("%s, %s grid (cell %.6g, %d x %d x %d): smallest d2 / lb %.6f over cells, %.6f over outer faces" %
              (C.label(case), policy, lay.cell, *lay.dims, cell_ratio, face_ratio))
        assert holds and cell_ratio >= 1.0 and face_ratio >= 1.0


def test_the_product_cell_times_cell_breaks_the_bound():
    """Why the bound is multiplied by the cell twice and not by cell * cell: with that float32 product the bound of a neighbouring cell is +inf (or 0 * inf = NaN)
    on wide_and_1e23, above thousands of finite float32 distances -- records the search then never looks at."""
    xyz = C.mixed("wide_and_1e23")
    lay = G.layout_of(xyz, "knn")
    u, c = G.cell_pos(xyz, lay), G.cells_of(xyz, lay)
    with np.errstate(over="ignore", invalid="ignore"):
        cell2 = np.float32(lay.cell) * np.float32(lay.cell)
        d2 = F.d2_f32(xyz[:256, None, :], xyz[None, :, :])
        gaps = [G.axis_gap(u[:256, None, k], c[None, :, k], c[None, :, k]) for k in range(3)]
        s = ((gaps[0] * gaps[0] + gaps[1] * gaps[1]).astype(np.float32) + gaps[2] * gaps[2]).astype(np.float32)
        lb32 = (s * cell2).astype(np.float32) * np.float32(G.LB_FACTOR)
        other = (c[None, :, :] != c[:256, None, :]).any(axis=2)
        assert np.isinf(cell2) and int((other & (lb32 > d2)).sum()) > 1000 and int((other & np.isnan(lb32)).sum()) > 100
        assert (G.grid_lb2(gaps[0], gaps[1], gaps[2], lay.cell) <= d2).all()


@pytest.mark.parametrize("case", [("uniform", e) for e in C.EXTREME] + list(C.MIXED), ids=C.label)
def test_ball_box_holds_every_neighbour(case):
    """radius_query and radius_axis_cells restated (tests/test_pointgrid_layout_cpu.py has the same on its scenes): every neighbour
    (d2 < r2) of every record lies in the box of cells the walk visits, in a row it does not skip -- the record itself too, where
    float32(q - origin) has overflowed and its position says nothing."""
    xyz = C.cloud_of(case)
    mn, mx, nfin = G.box_of(xyz)
    for r in (C.outside_radius(case), 1e30):
        lay = G.layout(mn, mx, nfin, "radius", r)
        reach, r2, cell = G.radius_reach(r, lay), R.r2_f32(r), lay.cell
        u, c = G.bound_pos(G.cell_pos(xyz, lay)), G.cells_of(xyz, lay)
        box = [G.radius_axis_cells(u[:, k], reach, lay.dims[k]) for k in range(3)]
        pairs = 0
        for s in range(0, len(xyz), 256):
            q = slice(s, s + 256)
            with np.errstate(over="ignore", under="ignore"):
                nb = F.d2_f32(xyz[q, None, :], xyz[None, :, :]) < r2
            inside = np.ones_like(nb)
            for k in range(3):
                inside &= (c[None, :, k] >= box[k][0][q, None]) & (c[None, :, k] <= box[k][1][q, None])
            gx = G.axis_gap(u[q, 0], box[0][0][q], box[0][1][q])[:, None]
            gy = G.axis_gap(u[q, None, 1], c[None, :, 1], c[None, :, 1])
            gz = G.axis_gap(u[q, None, 2], c[None, :, 2], c[None, :, 2])
            row_lb = G.grid_lb2(np.broadcast_to(gx, gy.shape), gy, gz, cell)
            assert (inside | ~nb).all(), (case, r)
            assert (~(row_lb > r2) | ~nb).all(), (case, r)
            pairs += int(nb.sum())
        print("%s, r = %.6g: cell %.6g, %d x %d x %d, reach %.4g cells, %d neighbour pairs, all inside" %
              (C.label(case), r, lay.cell, *lay.dims, reach, pairs))
        assert pairs >= len(xyz) or r2 == 0
    if case == "two_at_3e38":                                 # the record at +3e38: its position has overflowed, its box is the whole x axis
        assert np.isnan(u[1500, 0]) and (box[0][0][1500], box[0][1][1500]) == (0, lay.dims[0] - 1)


@pytest.mark.parametrize("case", C.FAR_TARGETS, ids=C.label)
def test_bound_holds_for_sources_far_outside_the_target(case):
    """The queries of a fitness score are not points of the index: a source record may lie any number of cells outside the
    target's box.  Up to kPosMax cells the gaps are finite and the bound is below every float32 distance; beyond, the position is a
    NaN and every gap 0."""
    tgt, src = C.cloud_of(case), C.far_source(case)
    lay = G.layout_of(tgt, "fit")
    u = G.cell_pos(src, lay)
    with np.errstate(invalid="ignore"):
        far = np.abs(u).max(axis=1)
    cell_ratio, face_ratio, holds = _bounds(tgt, lay, src)
    print("%s: cell %.6g, sources up to %.3g cells from the origin, %d beyond kPosMax; smallest d2 / lb %.6f over cells, %.6f over outer faces" %
          (C.label(case), lay.cell, far.max(), int((far > G.POS_MAX).sum()), cell_ratio, face_ratio))
    assert holds and cell_ratio >= 1.0 and face_ratio >= 1.0
    assert (far > G.POS_MAX).sum() >= 3 and ((far > 1e9) & (far <= G.POS_MAX)).sum() >= 3
    d = F.nearest_d2_brute(src, tgt)
    assert np.isfinite(d[far > G.POS_MAX]).any() or case[1] >= 0      # a finite distance from beyond kPosMax: a tiny target box


# ------------------------------------------------------------------------------------------------ the left-out share
@pytest.mark.parametrize("name", ["uniform", "sphere"])
def test_share_left_out_by_the_gap_condition(name):
    for k in C.NORMAL_KS:
        ref = N.normals(C.base(name), k, knn_result=C.knn_ref(C.brute(name, 0), k))
        out = 1.0 - float((ref.gap[ref.finite] >= 1e-3).mean())
        print("%s k=%d: %.2f %% of the records left out by gap_ratio >= 1e-3" % (name, k, 100 * out))
        assert out <= 0.05


# uniform at 2^e, k = 10, the scale-1 normals: (rows with a denormal d2, rows with a +inf d2, rows with a NaN, all-zero rows)
FPFH_REGIME = {-120: (0, 0, 0, 1500), -70: (1500, 0, 1500, 0), -62: (1500, 0, 1500, 0), 62: (0, 0, 0, 0), 66: (0, 4, 0, 0), 70: (0, 1500, 0, 1484),
               100: (0, 1500, 0, 1500)}


def test_fpfh_regimes_outside_the_window():
    """What the FPFH contract gives where a d2 is not a finite normal float, on the reference alone.  All d2 zero: every neighbour is
    skipped, 33 zeros.  A denormal d2: w = 1.0f / d2 = +inf, val = SPFH * w is +inf or 0 * inf = NaN, and the row of a FINITE record
    with finite normals holds NaNs -- nan_rows (non-finite records and normals) does not name it, is_dense has to.  A +inf d2:
    w = 0, the neighbour adds nothing, no NaN; all ten at +inf (or 0, the record itself): 33 zeros."""
    assert sorted(FPFH_REGIME) == sorted(C.EXTREME)
    nrm = np.ascontiguousarray(fpfh_cases.ref_normals("uniform"))
    for e in C.EXTREME:
        xyz = C.cloud_of(("uniform", e))
        r = fpfh_ref.fpfh(xyz, nrm, 10, knn_result=C.knn_ref(C.brute("uniform", e), 10))
        denormal = ((r.d2 > 0) & (r.d2 < C.FLT_MIN)).any(axis=1)
        inf = np.isinf(r.d2).any(axis=1)
        nan = np.isnan(r.fpfh).any(axis=1)
        zero = (r.fpfh == 0).all(axis=1)
        got = (int(denormal.sum()), int(inf.sum()), int(nan.sum()), int(zero.sum()))
        print("uniform*2^%d: rows with a denormal d2 %d, with a +inf d2 %d, with a NaN %d, all zero %d" % ((e,) + got))
        assert got == FPFH_REGIME[e], (e, got)
        assert not r.nan_rows.any() and not r.fragile_nb.any()
        assert (nan == denormal).all() and (np.isnan(r.fpfh).all(axis=1) == nan).all()   # a NaN anywhere in a row is a NaN everywhere in it
        assert fpfh_ref.blocks_ok(r.fpfh[~nan]).all()
        if e == -120:
            assert (r.d2 == 0).all() and (r.spfh != 0).any()                  # (the pair features are doubles: the SPFH rows are not zero)


def test_fpfh_condition_holds_at_2_to_the_62():
    """The GPU test compares FPFH outside the window where every d2 among the ten nearest is a finite normal float: at 2^62 it is,
    on every base cloud."""
    for name in C.BASES:
        d10 = C.brute(name, 62).d2[S.finite_rows(C.base(name))][:, :10]
        assert (np.isfinite(d10) & ((d10 == 0) | (d10 >= C.FLT_MIN))).all()
