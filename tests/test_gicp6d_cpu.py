"""GICP6D without a GPU: the colour conversion's host half (rsreg_lab_tables, rsreg_rgb_to_lab) against tests/gicp6d_ref.py, and
the scene the GPU test aligns, pinned here by the reference ALONE.

Tables: every entry within one float32 ulp of the float64 formula (the library computes it in double and rounds once; pow and cbrt
of two C libraries may differ in the last bit of the double, which can move the rounded float by one ulp at most), both tables
non-decreasing.  Conversion: behind the tables it is float multiplies, adds and divides rounded once each, so the library's floats
equal the reference's fed the library's own tables, bit for bit.

The scene (tests/gicp6d_cases.py): the 6-D reference ends within 1e-3 Frobenius of the truth, the 3-D reference of
tests/gicp_ref.py stays more than 5e-3 away on the same inputs, and the 6-D result moves by less than 1e-5 when every sum is
perturbed by 1e-12 relative -- the margin argument of tests/test_gicp_cpu.py: the engine's sums differ from the reference's by
the order of their additions only, far below that perturbation, so 1e-4 between engine and reference on the GPU is a bound with
room, not a fit.
"""
import ctypes as C

import numpy as np
import pytest

import gicp6d_cases as GC6
import gicp6d_ref as R


@pytest.fixture(scope="module")
def api(rs):
    from rsreg_amd import api, lib
    lib.build()
    return api


def _ulp_distance(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)   # (all entries are positive floats)


def test_tables_are_the_float64_formula_to_an_ulp_and_monotone(api):
    S, F = api.lab_tables()
    S64, F64 = R.tables64()
    assert S.dtype == np.float32 and S.shape == (256,) and F.shape == (4000,)
    assert _ulp_distance(S, S64.astype(np.float32)).max() <= 1 and _ulp_distance(F[1:], F64.astype(np.float32)[1:]).max() <= 1
    assert (np.diff(S) >= 0).all() and (np.diff(F) >= 0).all()
    assert S[0] == 0.0 and S[255] == 1.0 and F[0] == np.float32(16.0 / 116.0)
    from rsreg_amd import lib
    assert lib.lib().rsreg_lab_tables(None, None) == lib.RSREG_ERR_INVALID_ARG


def _check(api, rgba):
    S, F = api.lab_tables()
    got = api.rgb_to_lab(rgba)
    want = R.lab(S, F, rgba)
    assert got.tobytes() == want.tobytes(), np.flatnonzero((got != want).any(axis=1))[:8]
    return got


def test_rgb_to_lab_is_the_reference_bit_for_bit(api):
    v = np.arange(0, 256, 17, dtype=np.uint32)
    r, g, b = np.meshgrid(v, v, v, indexing="ij")
    lab = _check(api, GC6.pack_rgb(r.ravel(), g.ravel(), b.ravel()))
    assert len(lab) == 4096
    # the ranges of the normalised coordinates over the sRGB cube's corners and grid: L' in [0, 1], |a'|, |b'| within 1
    assert lab[:, 0].min() == 0.0 and lab[:, 0].max() <= 1.0 and np.abs(lab[:, 1:]).max() <= 1.0
    rng = np.random.default_rng(5)
    _check(api, rng.integers(0, 1 << 32, 100_000, dtype=np.uint64).astype(np.uint32))   # (the top byte is not read)
    black = _check(api, np.array([0], np.uint32))
    assert (black == 0).all()
    assert (api.rgb_to_lab(np.array([0xff000000], np.uint32)) == 0).all()
    _check(api, np.array([0xffffff], np.uint32))


def test_white_and_the_five_clamps(api):
    """The table index clamps at 3999 (white: y = 1.0000001 -> index 4000 unclamped) and at 0 (never below: v >= 0); L caps at 100
    and a, b clamp at +-120 only with tables other than the library's (test_every_colour_of_the_cube: no colour gets there), so those
    three are shown on the reference, through a table made for the purpose."""
    S, F = api.lab_tables()
    white = np.array([0xffffff], np.uint32)
    x = (S[255] * np.float32(0.412453) + S[255] * np.float32(0.357580)) + S[255] * np.float32(0.180423)
    y = (S[255] * np.float32(0.212671) + S[255] * np.float32(0.715160)) + S[255] * np.float32(0.072169)
    assert int(np.float32(y) * np.float32(4000.0)) >= 4000 or int((x / np.float32(0.95047)) * np.float32(4000.0)) >= 4000
    lab = _check(api, white)
    assert lab[0, 0] == (np.float32(116.0) * F[3999] - np.float32(16.0)) / np.float32(100.0)
    # index 0: black
    assert (_check(api, np.array([0], np.uint32)) == 0).all()
    # L > 100, a > 120, a < -120, b > 120, b < -120: no colour reaches them through the library's tables (the exhaustive test below
    # never sees |a'|, |b'| or L' at 1), so the reference shows them through a table that exaggerates f() from a quarter up:
    # white caps L; red has vx above the step and vy below it, a mid green the reverse (and vz below), blue vz above and vy below
    Fbig = F.copy()
    Fbig[1000:] = np.float32(3.0)
    hit = R.lab(S, Fbig, np.array([0xffffff, 0xff0000, 0x00aa00, 0x0000ff], np.uint32))
    assert hit[0, 0] == 1.0 and hit[1, 1] == 1.0 and hit[2, 1] == -1.0 and hit[2, 2] == 1.0 and hit[3, 2] == -1.0
    assert (np.abs(hit) <= 1.0).all()
    from rsreg_amd import lib
    assert lib.lib().rsreg_rgb_to_lab(None, 3, None) == lib.RSREG_ERR_INVALID_ARG
    assert lib.lib().rsreg_rgb_to_lab(None, 0, None) == 0


def test_every_colour_of_the_cube(api):
    """all 2^24 colours, the library against the reference: the same bytes; L' within [0, 1), |a'| and |b'| below 1"""
    S, F = api.lab_tables()
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for r in range(0, 256, 32):
        rgba = np.arange(r << 16, (r + 32) << 16, dtype=np.uint32)
        got = api.rgb_to_lab(rgba)
        assert got.tobytes() == R.lab(S, F, rgba).tobytes(), r
        lo, hi = np.minimum(lo, got.min(axis=0)), np.maximum(hi, got.max(axis=0))
    print("L' in [%.6f, %.6f], a' in [%.6f, %.6f], b' in [%.6f, %.6f]" % (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]))
    assert lo[0] == 0.0 and hi[0] < 1.0 and lo[1] > -1.0 and hi[1] < 1.0 and lo[2] > -1.0 and hi[2] < 1.0


def test_brute_force_rules():
    q = np.array([[0, 0, 0], [0, 0, 0], [np.nan, 0, 0], [0, 0, 0]], np.float32)
    qc = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [np.inf, 0, 0]], np.float32)
    t = np.array([[0.01, 0, 0], [0.01, 0, 0], [0.02, 0, 0], [np.nan, 0, 0], [0.0, 0, 0]], np.float32)
    tc = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0], [np.nan, 0, 0]], np.float32)
    idx, d2 = R.nearest6(q, qc, t, tc, 1.5)
    # exact copies: the lowest index; the colour decides against the nearer point; a NaN candidate is skipped (records 3, 4);
    # a query whose position or colour is not finite has no pair
    assert idx.tolist() == [0, 2, -1, -1] and d2[0] == np.float32(0.01) ** 2 and d2[1] == np.float32(0.02) ** 2
    idx, _ = R.nearest6(q[:2], qc[:2], t, tc, 0.015)
    assert idx.tolist() == [0, -1]   # 3-D distance 0.01 inside the gate, 6-D distance outside
    # weight 0 is the 3-D search
    import plane_ref
    xyz_s, lab_s = GC6.box_cloud(300, 1)
    xyz_t, lab_t = GC6.box_cloud(400, 2)
    i6, d6 = R.nearest6(xyz_s, R.scaled(lab_s, 0.0), xyz_t, R.scaled(lab_t, 0.0), 1e3)
    i3, d3 = plane_ref.nearest_brute(xyz_s, xyz_t)
    assert (i6 == i3).all() and (d6 == d3).all()


def test_the_scene_needs_colour_and_the_reference_finds_the_pose():
    c = GC6.scene()
    ls, lt = GC6.scene_lab()
    r6, r3 = GC6.scene_reference6(), GC6.scene_reference3()
    e6 = float(np.linalg.norm(r6.T.astype(np.float64) - c.truth))
    e3 = float(np.linalg.norm(r3.T.astype(np.float64) - c.truth))
    start = float(np.linalg.norm(np.eye(4) - c.truth))
    print("scene: 6-D %d iterations (%s) |T - truth|_F %.3g; 3-D %d iterations (%s) %.3g; start %.3g; per iteration 6-D %s"
          % (r6.iterations, r6.state, e6, r3.iterations, r3.state, e3, start, ["%.2g" % e for e in r6.errors]))
    assert r6.converged and r6.state == "TRANSFORM" and r6.iterations < c.prm.max_iterations and r6.n_correspondences == len(c.src)
    assert r3.converged and r3.state == "TRANSFORM"
    assert e6 < 1e-3
    assert e3 > 5e-3
    moved = []
    for seed in (1, 2):
        got = R.gicp6d(c.src, c.tgt, ls, lt, c.cov_s, c.cov_t, GC6.SCENE_WEIGHT, None, c.prm, perturb=(np.random.default_rng(seed), 1e-12))
        moved.append(float(np.linalg.norm(got.T.astype(np.float64) - r6.T.astype(np.float64))))
    print("scene: sums perturbed by 1e-12 move the 6-D transform by %s" % ["%.3g" % m for m in moved])
    assert max(moved) < 1e-5


def test_struct_sizes_and_refusals_without_a_context(api):
    from rsreg_amd import lib
    L = lib.lib()
    assert C.sizeof(lib.GicpParams) == 48 and L.rsreg_version() == 4
    assert L.rsreg_gicp6d_begin(None, None, None, 0.032) == lib.RSREG_ERR_INVALID_ARG
    assert L.rsreg_gicp_set_source_lab(None, None, 0, 12) == lib.RSREG_ERR_INVALID_ARG
    assert L.rsreg_gicp_set_target_lab(None, None, 0, 12) == lib.RSREG_ERR_INVALID_ARG
