"""CPU: the references of the two voxel filters across the float32 range (tests/voxel_scale_cases.py holds the clouds;
tests/test_voxel_scale_gpu.py asks the kernels).

  * tests/approx_voxel_ref.py, written from the rules in include/rsreg.h, reproduces the three outputs of the approx_voxel golden
    fixture byte for byte, and equals the sequential host filter (rsreg_approx_voxel_grid) and the oracle (orc.approx_voxel_grid)
    on every case of (a) to (d).
  * tests/voxelgrid_ref.py equals rsreg_voxel_grid on (a), (d) and (e): records and info.
  * The window: at every exponent of EXPONENTS no input, partial sum or output of either reference overflows or is a denormal,
    and the reference output at 2^e is the scale-1 output with xyz moved by exactly 2^e, w and rgba unchanged, the VoxelGrid info
    equal.  None of the four candidates (-100, -40, 40, 100) had to be dropped.
  * Each case of (b) to (e) does, on the reference, what it is there for: a case that no longer does fails here."""
import ctypes as C

import numpy as np
import pytest

import approx_voxel_ref as A
import voxel_scale_cases as S
import voxelgrid_cases as V
import voxelgrid_ref as R

F = np.float32
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib(rs):
    from rsreg_amd import lib as L
    L.build()
    return L


def same_bytes(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ------------------------------------------------------------------------------------------------ the references against the host code
def test_reference_reproduces_the_golden_fixture(golden):
    g = golden("approx_voxel")
    for key_in, key_out, leaf in (("in", "leaf_001", 0.01), ("in", "leaf_1", 1.0), ("wide_in", "wide_leaf_01", 0.1)):
        out = A.approx_voxel_grid(g[key_in], (leaf, leaf, leaf))
        assert len(out) == len(g[key_out]) > 0
        for f in ("x", "y", "z", "w", "rgba"):                          # (the 12 padding bytes of the fixture's records were never defined)
            np.testing.assert_array_equal(out[f].view(np.uint32), g[key_out][f].view(np.uint32))
        assert not out.view(np.uint8).reshape(len(out), -1)[:, 20:].any()


@pytest.mark.parametrize("case", S.APPROX_ALL, ids=S.label)
def test_approx_host_and_oracle_equal_reference(lib, orc, case):
    pts, leaf = S.approx_case(*case)
    want = S.approx_reference(*case)
    same_bytes(S.approx_host(lib, pts, leaf), want)
    assert S.same_fields(orc.approx_voxel_grid(R.raw_copy(pts), leaf), want)      # (the wrapper's copy leaves the padding undefined)


@pytest.mark.parametrize("case", S.GRID_ALL, ids=S.label)
def test_grid_host_equals_reference(lib, case):
    pts, leaf, all_data, mp = S.grid_case(*case)
    want, want_info = S.grid_reference(*case)
    got, info = V.run_host(lib, pts, leaf, all_data, mp)
    assert info == want_info
    same_bytes(got, want)


def test_refused_leaves(lib):
    pts = np.ascontiguousarray(S.grid_cases()["far_1e9"][0])
    out, n_out = np.zeros_like(pts), C.c_size_t(0)
    for leaf in S.REFUSED_LEAVES:
        with np.errstate(over="ignore"):
            assert leaf > 0 and np.isinf(F(1.0) / F(leaf))
        for lf in ((leaf, 1.0, 1.0), (1.0, 1.0, leaf)):
            lf = np.asarray(lf, F)
            assert lib.lib().rsreg_voxel_grid(pts.ctypes.data, len(pts), 32, lf.ctypes.data, 1, 0, out.ctypes.data, C.byref(n_out), None) == lib.RSREG_ERR_INVALID_ARG
            with pytest.raises(AssertionError), np.errstate(over="ignore"):
                R.leaf_grid(pts, lf)
    smallest = S.grid_cases()["leaf_2m127"][1][0]
    assert S.is_denormal(smallest) and F(1.0) / F(smallest) == F(2.0 ** 127)
    assert S.is_denormal(F(1.0) / F(S.FLT_MAX))


# ------------------------------------------------------------------------------------------------ (a) the window
@pytest.mark.parametrize("name", sorted(S.SCALED))
def test_window(name):
    a0, (g0, info0) = S.approx_reference("scaled", name, 0), S.grid_reference("scaled", name, 0)
    assert len(a0) > 10 and len(g0) > 10
    assert sum(e < 0 for e in S.EXPONENTS) >= 2 and sum(e > 0 for e in S.EXPONENTS) >= 2
    for e in S.EXPONENTS:
        pts, leaf = S.scaled(name, e)
        ae, (ge, infoe) = S.approx_reference("scaled", name, e), S.grid_reference("scaled", name, e)
        sums = S.partial_sums(pts, S.approx_runs("scaled", name, e)) + S.partial_sums(pts, S.grid_runs(pts, leaf))
        for what in [pts[f] for f in "xyz"] + [ae[f] for f in "xyz"] + [ge[f] for f in "xyz"] + sums + [np.asarray(leaf, F), F(1.0) / np.asarray(leaf, F)]:
            assert np.isfinite(what).all() and not S.is_denormal(what).any(), (name, e)
        same_bytes(ae, S.moved(a0, e))
        same_bytes(ge, S.moved(g0, e))
        assert infoe == info0


def test_scaled_clouds_cover_what_they_claim():
    """run_classes under the approximate filter: leaf l is voxel (l, 0, 0) in slot 3 l, one run per class, interleaved in the input;
    the boundary cloud: many runs per slot"""
    the_runs = S.approx_runs("scaled", "run_classes", 0)
    assert sorted(len(m) for _, m in the_runs) == sorted(V.RUN_LENGTHS)
    ijk = np.asarray([v for v, _ in the_runs])
    assert (ijk[:, 0] == np.arange(len(V.RUN_LENGTHS))).all() and (ijk[:, 1:] == 0).all()       # (emitted at the end: in slot order)
    assert (A.slot_of(ijk[:, 0], ijk[:, 1], ijk[:, 2]) == 3 * ijk[:, 0]).all()
    for name in ("boundaries_l003", "boundaries_aniso"):
        ijk = np.asarray([v for v, _ in S.approx_runs("scaled", name, 0)])
        slots = A.slot_of(ijk[:, 0], ijk[:, 1], ijk[:, 2])
        assert len(slots) > 4 * len(set(slots.tolist())) and (ijk < 0).any()


# ------------------------------------------------------------------------------------------------ (b) cell indices at and past int32
def _merged_run(the_runs, pts, axis):
    """the runs whose cell index on `axis` is INT32_MIN and that hold both signs of that coordinate"""
    f = "xyz"[axis]
    return [m for v, m in the_runs if v[axis] == INT32_MIN and (pts[f][m] > 0).any() and (pts[f][m] < 0).any()]


@pytest.mark.parametrize("name", [n for n in S.approx_cases() if n.startswith(("cell_l1_", "cell_l001_"))])
def test_cell_cases_merge_at_int32_min(name):
    pts, leaf = S.approx_cases()[name]
    the_runs = S.approx_runs("cell", name)
    axes = {"x": (0,), "y": (1,), "xyz": (0, 1, 2)}[name.split("_")[-1]]
    for a in axes:
        f = "xyz"[a]
        merged = _merged_run(the_runs, pts, a)
        assert merged, name                                              # the INT32_MIN merge happened: +big and -big in one run
        with np.errstate(over="ignore", invalid="ignore"):
            c = np.floor(pts[f] * (F(1.0) / F(leaf[a])))
        past = ~((c >= F(-2.0 ** 31)) & (c < F(2.0 ** 31))) & A.finite_rows(pts)
        assert past.sum() >= 20 and (A.cells(pts, leaf)[past, a] == INT32_MIN).all()
    # emission order matters: most runs are flushed by a record, not at the end, and runs of the merged voxel are among them
    flushed = len(the_runs) - len({int(A.slot_of(*v)) for v, _ in the_runs})
    assert flushed > len(the_runs) // 3
    assert sum(1 for v, _ in the_runs if v[axes[0]] == INT32_MIN) >= 3
    assert np.isfinite(np.stack([S.approx_reference("cell", name)[f] for f in "xyz"])).any()


def test_cell_case_values():
    """leaf 1: the largest float below 2^31 keeps its own cell, -2^31 is INT32_MIN by value, everything else by the rule"""
    got = A.cell_index(np.asarray(S.PAST_INT32, F), 1.0).tolist()
    assert got == [2147483520] + [INT32_MIN] * 9
    assert A.cell_index(np.asarray([3e7, -3e7, 2.1e7], F), 0.01).tolist() == [INT32_MIN, INT32_MIN, 2100000000]
    assert A.cell_index(np.asarray([0.0, -0.0, 1.0, -1.0], F), 2.0 ** -140).tolist() == [INT32_MIN] * 4        # NaN, NaN, +inf, -inf
    assert int(A.slot_of(INT32_MIN, 0, 0)) == 0 and int(A.slot_of(INT32_MIN, INT32_MIN, INT32_MIN)) == 0
    assert int(A.slot_of(INT32_MAX, 0, 0)) != 0                                                                 # (a saturating conversion lands elsewhere)


def test_extreme_leaves_of_the_approximate_filter():
    pts, leaf = S.approx_cases()["cell_leaf_2m140"]
    with np.errstate(over="ignore"):
        assert np.isinf(F(1.0) / F(leaf[0]))
    the_runs = S.approx_runs("cell", "cell_leaf_2m140")
    assert len(the_runs) == 1 and the_runs[0][0] == (INT32_MIN,) * 3 and len(the_runs[0][1]) == len(pts)    # one voxel: NaN, +inf and -inf alike
    assert (pts["x"] == 0).sum() > 20 and np.signbit(pts["x"][pts["x"] == 0]).any() and (pts["x"] > 0).any() and (pts["x"] < 0).any()
    x_only = S.approx_runs("cell", "cell_leaf_2m140_x_only")
    assert len(x_only) > 30 and all(v[0] == INT32_MIN for v, _ in x_only)
    pts, leaf = S.approx_cases()["cell_leaf_3e38"]
    assert S.is_denormal(F(1.0) / F(leaf[0]))
    ijk = A.cells(pts, leaf)
    assert set(np.unique(ijk).tolist()) == {-2, -1, 0, 1} and (np.abs(pts["x"]) > 1e37).sum() > 30


# ------------------------------------------------------------------------------------------------ (c) cancelling runs
@pytest.mark.parametrize("name", sorted(S.CANCEL))
def test_cancelling_runs(name):
    n, zero_at, _ = S.CANCEL[name]
    pts, leaf = S.approx_cases()[name]
    the_runs = S.approx_runs("cell", name)
    big = [m for v, m in the_runs if v == (INT32_MIN, 0, 0)]
    assert len(big) == 1 and len(big[0]) == n and len(the_runs) > 5      # ONE run of the merged voxel, among other runs
    x = pts["x"][big[0]]
    assert (np.abs(x) >= F(2.0 ** 31)).all() and (np.sign(x[::2]) > 0).all() and (np.sign(x[1::2]) < 0).all()
    part = np.cumsum(x, dtype=F)
    assert np.isfinite(part).all()
    for z in zero_at:
        assert part[z] == 0                                              # a partial sum is exactly zero
    assert (np.diff(np.sign(part)) != 0).sum() >= min(3, n // 2)         # the running sum crosses zero
    binades = {int(b) for b in np.frexp(part[part != 0])[1]}
    assert len(binades) >= (3 if n == 5 else 8)
    if name.endswith("window_ends_at_zero"):
        assert 1023 in zero_at and part[1023] == 0 and part[1022] != 0   # the first window of 1 024 points ends at a zero sum
    inexact = sum(float(part[i]) != float(part[i - 1]) + float(x[i]) for i in range(1, n))
    assert inexact >= (1 if n == 5 else n // 10)                         # the additions round: the order of the sum matters


# ------------------------------------------------------------------------------------------------ (d) sums that leave the normal range
@pytest.mark.parametrize("name", sorted(S.range_cases()))
def test_range_cases(name):
    pts, leaf = S.range_cases()[name]
    kind, n = name.rsplit("_", 1)
    a_runs, g_runs = S.approx_runs("range", name), S.grid_runs(pts, leaf)
    assert len(a_runs) == len(g_runs) == 1 and len(a_runs[0][1]) == len(g_runs[0][1]) == int(n)     # one voxel, one leaf
    sums = np.stack(S.partial_sums(pts, a_runs))
    a_out, (g_out, info) = S.approx_reference("range", name), S.grid_reference("range", name)
    assert len(a_out) == len(g_out) == 1 and info["n_leaves"] == 1 and not info["overflowed"]
    for f in "xyz":
        assert a_out[f].tobytes() == g_out[f].tobytes()
    xyz_out = np.asarray([a_out[f][0] for f in "xyz"])
    if kind in ("plus_3e38", "minus_3e38"):
        inf = F(np.inf) if kind == "plus_3e38" else F(-np.inf)
        assert np.isfinite(sums[:, 0]).all() and (sums[:, 1:] == inf).all() and (xyz_out == inf).all()      # +-inf from the second term on
        assert not S.is_denormal(F(1.0) / F(leaf[0]))
    elif kind == "denormal_stays":
        assert S.is_denormal(np.stack([pts[f] for f in "xyz"])).all() and S.is_denormal(sums).all() and S.is_denormal(xyz_out).all()
    elif kind == "denormal_crosses":
        assert S.is_denormal(np.stack([pts[f] for f in "xyz"])).all() and S.is_denormal(sums[:, 0]).all()
        assert (sums[:, -1] >= F(S.FLT_MIN)).all() and S.is_denormal(xyz_out).all()
    else:
        assert pts["x"][0] == F(1e30) and (pts["x"][1:] == 1).all() and (sums[0] == F(1e30)).all()             # the ones are absorbed
        assert pts["y"][int(n) // 2] == F(1e30) and xyz_out[0] == F(1e30) / F(int(n))


# ------------------------------------------------------------------------------------------------ (e) far and wide boxes
def test_far_boxes_cover_what_they_claim():
    info = {k: S.grid_reference("far", k)[1] for k in S.grid_cases()}
    out = {k: S.grid_reference("far", k)[0] for k in S.grid_cases()}
    far = info["far_1e9"]
    assert far["min_b"][0] == 10 ** 9 and far["max_b"][0] == 10 ** 9 + 512 and far["n_leaves"] == 3             # large but exact
    for k in ("far_plus_3e9", "far_plus_3e9_nan", "far_minus_3e9", "far_plus_3e9_y", "far_plus_3e9_xyz_only"):
        a = 1 if k.endswith("_y") else 0
        sat = INT32_MIN if "minus" in k else INT32_MAX
        assert info[k]["min_b"][a] == info[k]["max_b"][a] == sat and info[k]["div_b"] == [1, 1, 1], k            # both bounds saturated
        assert info[k]["n_leaves"] == info[k]["n_out"] == 3 and not info[k]["overflowed"], k
    pts, leaf = S.grid_cases()["far_plus_3e9"][:2]
    assert [i for i, _ in S.grid_runs(pts, leaf)] == [852516352, 852516608, 852516864]                          # keys far above prod(div_b) - 1 = 0
    for k in ("far_max_b_only", "far_max_b_only_nan", "far_max_b_only_y"):
        a = 1 if k.endswith("_y") else 0
        assert info[k]["min_b"][a] == 2147483520 and info[k]["max_b"][a] == INT32_MAX and info[k]["div_b"][a] == 128, k
        assert info[k]["n_leaves"] == 3, k
        pts, leaf = S.grid_cases()[k][:2]
        assert max(i for i, _ in S.grid_runs(pts, leaf)) >= 128 * (1 if a == 0 else 1)                          # ijk = 128, 384: past div_b
    for k in S.grid_cases():
        if k.endswith("_nan"):
            assert info[k]["n_finite"] == len(S.grid_cases()[k][0]) - 1, k
    m2 = info["far_minus_3e9_min2"]
    assert m2["n_leaves"] == 4 and m2["n_out"] == 3 and m2["min_b"][0] == INT32_MIN
    assert (out["far_plus_3e9_xyz_only"]["rgba"] == 0xff000000).all() and (out["far_plus_3e9_nan"]["rgba"] != 0xff000000).any()
    r = info["last_division_rounds_up"]
    assert r["min_b"][0] == -1 and r["div_b"][0] == 2 ** 25 and r["div_b"][1:] == [1, 1] and r["n_leaves"] == 3
    pts, leaf = S.grid_cases()["last_division_rounds_up"][:2]
    assert [i for i, _ in S.grid_runs(pts, leaf)] == [0, 6, 2 ** 25]                                            # a key of 26 bits, prod(div_b) - 1 has 25
    pts, leaf = S.grid_cases()["leaf_of_negative_zeros"][:2]
    alone = [m for _, m in S.grid_runs(pts, leaf) if np.signbit(pts["x"][m]).all() and (pts["x"][m] == 0).all()]
    zero = out["leaf_of_negative_zeros"][(out["leaf_of_negative_zeros"]["x"] == 0)]
    assert len(alone) == 1 and len(alone[0]) == 4 and len(zero) == 1 and not np.signbit(zero["x"][0]) and not np.signbit(zero["y"][0])
    both = info["plus_and_minus_flt_max"]
    pts = S.grid_cases()["plus_and_minus_flt_max"][0]
    assert both["overflowed"] == 1 and both["n_out"] == len(pts) and out["plus_and_minus_flt_max"].tobytes() == pts.tobytes()
    with np.errstate(over="ignore"):
        assert np.isinf(F(S.FLT_MAX) - F(-S.FLT_MAX))
    assert info["at_1e30_leaf_1e28"]["min_b"][0] >= 50 and 10 < info["at_1e30_leaf_1e28"]["n_leaves"] <= 40
    assert info["leaf_2m127"]["min_b"] == [0, 0, 0] and info["leaf_2m127"]["max_b"] == [5, 5, 5] and info["leaf_2m127"]["n_leaves"] > 10
    assert S.is_denormal(S.grid_cases()["leaf_2m127"][0]["x"]).sum() > 10
    assert info["leaf_flt_max"]["min_b"] == [-1, -1, -1] and info["leaf_flt_max"]["max_b"] == [0, 0, 0] and info["leaf_flt_max"]["n_leaves"] == 8
