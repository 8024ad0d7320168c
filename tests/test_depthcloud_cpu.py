"""CPU: the host restatement of the capture step (rsreg_depth_to_cloud, csrc/depth_host.cpp) against the numpy reference written
from the contract (tests/depthcloud_ref.py): record bytes and width / height / is_dense, equal, on every case of
tests/depthcase_cases.py.  And the cases against the reference alone: each holds what it is there for."""
import ctypes as C

import numpy as np
import pytest

import depthcase_cases as D
import depthcloud_ref as R

F = np.float32


@pytest.fixture(scope="module")
def lib(rs):
    from rsreg_amd import lib as L
    L.build()
    return L


def same_bytes(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("name", sorted(D.cases()))
def test_host_restatement_equals_reference(lib, name):
    want, want_meta, _ = D.reference(name)
    got, meta = D.run_host(lib, D.cases()[name])
    assert meta == want_meta
    same_bytes(got, want)


def test_struct_layout(lib):
    assert C.sizeof(lib.Intrinsics) == 48 and C.sizeof(lib.DepthParams) == 192
    assert lib.DepthParams.color.offset == 48 and lib.DepthParams.rotation.offset == 96 and lib.DepthParams.depth_scale.offset == 144
    assert lib.DepthParams.r0.offset == 156 and lib.DepthParams.out_width.offset == 172 and lib.DepthParams.reserved.offset == 184


@pytest.mark.parametrize("w,h", [(13, 7), (848, 480), (640, 480), (4, 3), (1280, 720)])
def test_parameter_helpers(lib, w, h):
    """rsreg_depth_params_default is convert_to_pcl_new's shape, rsreg_depth_params_reference convert_to_pcl's"""
    q = lib.DepthParams()
    lib.lib().rsreg_depth_params_default(w, h, C.byref(q))
    assert D.params_dict(q) == R.params(w, h) and list(q.reserved) == [0, 0]
    lib.lib().rsreg_depth_params_reference(w, h, C.byref(q))
    got = D.params_dict(q)
    assert got == R.params_reference(w, h)
    assert (got["r0"], got["r1"], got["c0"], got["c1"]) == (h // 5, h // 5 * 4, w // 5, w // 5 * 4)
    assert (got["out_width"], got["out_height"], got["is_dense"]) == (w * 3 // 5, h * 3 // 5, 1)


def test_reference_crops_are_the_quirks_they_claim():
    p = D.cases()["reference_13x7"].p
    assert (p["c0"], p["c1"], p["out_width"], p["r0"], p["r1"], p["out_height"]) == (2, 8, 7, 1, 4, 4)
    out, meta, dbg = D.reference("reference_13x7")
    assert meta == (28, 32, 7, 4, 1) and len(dbg["d"]) == 18
    # the fill is linear: record 6 is the FIRST pixel of the window's second row, not the seventh of its first
    case = D.cases()["reference_13x7"]
    depth = D.depth_view(case)
    assert out["z"][6] == F(0.001) * F(depth[2, 2]) and out["z"][5] == F(0.001) * F(depth[1, 7])
    tail = out[18:]
    assert (tail["x"] == 0).all() and (tail["z"] == 0).all() and (tail["w"] == 1).all() and (tail["rgba"] == 0xff000000).all()
    assert not np.signbit(tail["x"]).any() and (out[:18]["rgba"] != 0xff000000).any()
    q = D.cases()["reference_848x480"].p
    assert q["c1"] - q["c0"] == 507 and q["out_width"] == 508 and q["r1"] - q["r0"] == 288 and q["out_height"] == 288
    assert D.reference("reference_848x480")[1] == (508 * 288, 32, 508, 288, 1)
    e = D.cases()["reference_640x480"].p
    assert (e["c1"] - e["c0"]) * (e["r1"] - e["r0"]) == e["out_width"] * e["out_height"] == 384 * 288


def test_cases_cover_what_they_claim():
    # -0 vertices: a zero depth under a ray with negative x or y
    for name in ("all_u16_scale_001", "all_u16_scale_odd", "ragged_67x131"):
        out = D.reference(name)[0]
        zero = out["z"] == 0
        assert (zero & np.signbit(out["x"])).any() and (zero & np.signbit(out["y"])).any(), name
        assert (zero & ~np.signbit(out["x"])).any() or name.startswith("all_u16")
    for name in ("all_u16_scale_001", "all_u16_scale_odd"):
        dbg = D.reference(name)[2]
        assert sorted(dbg["d"].tolist()) == list(range(65536))
        assert np.signbit(dbg["P"][dbg["d"] == 0][0, :2]).all()
    odd = D.cases()["all_u16_scale_odd"].p["depth_scale"]
    assert int(np.frexp(np.float64(odd))[0] * 2 ** 24) & 0xff and F(odd) != F(0.001)   # the mantissa's low bits are in use
    for name in ("all_u16_scale_001", "all_u16_scale_odd"):                            # ... and the products really round
        dbg, s = D.reference(name)[2], np.float64(D.cases()[name].p["depth_scale"])
        assert (dbg["P"][:, 2].astype(np.float64) != s * dbg["d"]).mean() > 0.5
    # the clamp, on all four sides
    dbg = D.reference("extrinsics_clamp")[2]
    cw, ch = 24, 20
    assert (dbg["ix"] < 0).any() and (dbg["ix"] > cw - 1).any() and (dbg["iy"] < 0).any() and (dbg["iy"] > ch - 1).any()
    assert ((dbg["ix"] >= 0) & (dbg["ix"] < cw) & (dbg["iy"] >= 0) & (dbg["iy"] < ch)).any()
    assert dbg["xi"].min() == 0 and dbg["xi"].max() == cw - 1 and dbg["yi"].min() == 0 and dbg["yi"].max() == ch - 1
    # truncation toward zero: a negative value above -1 is pixel 0, not -1
    assert ((dbg["tx"] > -1) & (dbg["tx"] < 0)).any() or ((dbg["ty"] > -1) & (dbg["ty"] < 0)).any()
    # the exact half
    dbg = D.reference("exact_half")[2]
    assert (dbg["tx"] == np.tile(np.arange(8, dtype=F) + F(0.5), 4)).all() and (dbg["xi"] == np.tile(np.arange(8), 4)).all()
    assert (dbg["ty"] == np.repeat(np.arange(4, dtype=F) + F(0.5), 8)).all()
    # q2 == 0: -inf, NaN and +inf reach the cast; all of them are pixel 0 (x86), not the last pixel
    out, _, dbg = D.reference("q2_zero")
    hit = dbg["d"] == D.Q2_DEPTH
    assert hit.any() and (dbg["q2"][hit] == 0).all() and (dbg["q2"][~hit & (dbg["d"] != 0)] != 0).all()
    for t, i, x in ((dbg["tx"], dbg["ix"], dbg["xi"]), (dbg["ty"], dbg["iy"], dbg["yi"])):
        assert np.isposinf(t[hit]).any() and np.isneginf(t[hit]).any() and np.isnan(t[hit]).any()
        assert (i[hit] == -2 ** 31).all() and (x[hit] == 0).all()
    color = D.color_view(D.cases()["q2_zero"])
    assert (color[0, 0] != color[0, -1]).any() and (color[0, 0] != color[-1, 0]).any()       # a saturating cast shows in the bytes
    # the default tail
    for name, n_tail in (("reference_13x7", 10), ("reference_848x480", 288), ("empty_window", 12), ("reference_640x480", 0)):
        out, _, dbg = D.reference(name)
        count = len(dbg["d"]) if dbg else 0
        assert len(out) - count == n_tail, name
        assert (out["rgba"][count:] == 0xff000000).all() and (out["w"] == 1).all()
    # colour of another size: pixels beyond the depth image's extent are looked up
    dbg = D.reference("color_32x18_depth_16x12")[2]
    assert dbg["xi"].max() > 15 and dbg["yi"].max() > 11
    # the distortions move vertices and colours
    case = D.cases()["distortion_both"]
    plain = dict(case.p, depth=dict(case.p["depth"], model=R.NONE), color=dict(case.p["color"], model=R.NONE))
    und = R.depth_to_cloud(D.depth_view(case), D.color_view(case), plain)[0]
    dis = D.reference("distortion_both")[0]
    assert (und["x"] != dis["x"]).any() and (und["rgba"] != dis["rgba"]).any()
    only_depth = R.depth_to_cloud(D.depth_view(case), D.color_view(case), dict(case.p, color=plain["color"]))[0]
    assert (only_depth["rgba"] != dis["rgba"]).any() and (only_depth["x"] == dis["x"]).all()
    # foreign models with zero coefficients act as none; so does none with coefficients
    for name in ("foreign_models_zero_coeffs", "none_ignores_coeffs"):
        case = D.cases()[name]
        plain = R.params(16, 12)
        assert D.reference(name)[0].tobytes() == R.depth_to_cloud(D.depth_view(case), D.color_view(case), plain)[0].tobytes()


@pytest.mark.parametrize("name", ["ragged_67x131", "padded_bpp3_bgr", "padded_bpp4_rgb", "color_32x18_depth_16x12"])
def test_channel_order_and_the_half_show_in_the_bytes(name):
    want = D.reference(name)[0]
    swapped = D.reference(name, swap_channels=True)[0]
    assert (want["rgba"] != swapped["rgba"]).any() and (want["x"].view(np.uint32) == swapped["x"].view(np.uint32)).all()
    r, b = (want["rgba"] >> 16) & 0xff, want["rgba"] & 0xff
    assert (((swapped["rgba"] >> 16) & 0xff) == b).all() and ((swapped["rgba"] & 0xff) == r).all()
    if name == "ragged_67x131":
        assert (want["rgba"] != D.reference(name, no_half=True)[0]["rgba"]).any()


def test_padding_is_not_read():
    """the padded cases give the records of the same images packed tightly"""
    for name in ("padded_bpp3_bgr", "padded_bpp4_rgb"):
        case = D.cases()[name]
        depth, color = D.depth_view(case), D.color_view(case)
        assert case.dstride > 2 * depth.shape[1] and case.cstride > case.p["bpp"] * color.shape[1]
        assert D.reference(name)[0].tobytes() == R.depth_to_cloud(depth.copy(), color.copy(), case.p)[0].tobytes()


def test_by_hand():
    """one pixel, worked by hand: d = 1000 at (c, r) = (3, 1), ppx = 1, ppy = 0, fx = fy = 2 -> ray (1, 0.5), z = 1 with scale 2^-10 * 1.024"""
    depth = np.zeros((2, 4), np.uint16)
    depth[1, 3] = 1024
    color = np.arange(2 * 4 * 3, dtype=np.uint8).reshape(2, 4, 3) + 100
    p = R.params(4, 2, depth=R.intrinsics(4, 2, 1, 0, 2, 2), color=R.intrinsics(4, 2, 1, 0, 2, 2), depth_scale=F(2.0 ** -10))
    out, w, h, dense, dbg = R.depth_to_cloud(depth, color, p)
    assert (w, h, dense, len(out)) == (4, 2, 0, 8)
    rec = out[1 * 4 + 3]
    assert (rec["x"], rec["y"], rec["z"], rec["w"]) == (1.0, 0.5, 1.0, 1.0)
    # back through the same camera: px = 1 * 2 + 1 = 3, py = 0.5 * 2 + 0 = 1; u * 4 + .5 = 3.5 -> 3, v * 2 + .5 = 1.5 -> 1
    b, g, r = color[1, 3]
    assert rec["rgba"] == 0xff000000 | (int(r) << 16) | (int(g) << 8) | int(b)
    # a zero depth: (u, v) = (0, 0), the colour of pixel (0, 0); x = (0 - 1) / 2 < 0 -> -0
    first = out[0]
    assert first["rgba"] == 0xff000000 | (int(color[0, 0, 2]) << 16) | (int(color[0, 0, 1]) << 8) | int(color[0, 0, 0])
    assert first["x"] == 0 and np.signbit(first["x"]) and first["y"] == 0 and not np.signbit(first["y"])
    p_rgb = dict(p, bgr=0)
    assert R.depth_to_cloud(depth, color, p_rgb)[0][7]["rgba"] == 0xff000000 | (int(b) << 16) | (int(g) << 8) | int(r)


def test_cast_rule():
    t = np.array([0.0, -0.0, 0.99, -0.99, 1.5, -1.5, 2147483520.0, 2147483648.0, -2147483648.0, -2147483904.0, np.inf, -np.inf, np.nan, 3e38], F)
    assert R.to_int(t).tolist() == [0, 0, 0, 0, 1, -1, 2147483520, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31]


@pytest.mark.parametrize("name", sorted(D.invalid()))
def test_refused_arguments(lib, name):
    p, dstride, cstride = D.invalid()[name]
    assert R.refused(p, dstride, cstride)
    case = D.cases()["tiny_7x5_identity"]
    assert not R.refused(case.p, case.dstride, case.cstride)
    out = np.full(64 * 32, 0x5a, np.uint8)
    q = D.c_params(lib, p)
    rc = lib.lib().rsreg_depth_to_cloud(case.dbuf.ctypes.data, dstride, case.cbuf.ctypes.data, cstride, C.byref(q), out.ctypes.data, 1 << 40, None, None, None)
    assert rc == lib.RSREG_ERR_INVALID_ARG
    assert (out == 0x5a).all()                                     # nothing written


def test_refused_pointers_and_capacity(lib):
    case = D.cases()["tiny_7x5_identity"]
    q = D.c_params(lib, case.p)
    out = np.zeros(35, R.POINT)
    f = lib.lib().rsreg_depth_to_cloud
    args = lambda **kw: [kw.get("d", case.dbuf.ctypes.data), case.dstride, kw.get("c", case.cbuf.ctypes.data), case.cstride, kw.get("q", C.byref(q)),
                         kw.get("o", out.ctypes.data), kw.get("cap", 35), None, None, None]
    assert f(*args()) == 0
    for kw in ({"d": None}, {"c": None}, {"q": None}, {"o": None}, {"cap": 34}):
        assert f(*args(**kw)) == lib.RSREG_ERR_INVALID_ARG, kw


def test_python_class_on_the_host(rs, lib):
    from rsreg_amd import api
    case = D.cases()["padded_bpp4_rgb"]
    want, meta, _ = D.reference("padded_bpp4_rgb")
    f = api.DepthToCloud()
    f.setDepthIntrinsics(**D.intr_kw(case.p["depth"]))
    f.setColorIntrinsics(**D.intr_kw(case.p["color"]))
    f.setExtrinsics(case.p["rotation"], case.p["translation"])
    f.setDepthScale(case.p["depth_scale"])
    f.setColorLayout(bytes_per_pixel=4, bgr=False)
    depth = np.lib.stride_tricks.as_strided(case.dbuf.view("<u2"), (12, 16), (case.dstride, 2))      # rows case.dstride bytes apart
    color = np.lib.stride_tricks.as_strided(case.cbuf, (12, 16, 4), (case.cstride, 4, 1))
    out = f.compute(depth, color)                                                                     # no context: the host restatement
    assert (out.width, out.height, out.is_dense) == meta[2:4] + (False,)
    same_bytes(out.points, want)
    # the reference crop through the class
    case = D.cases()["reference_13x7"]
    g = api.DepthToCloud()
    g.setDepthIntrinsics(**D.intr_kw(case.p["depth"]))
    g.setColorIntrinsics(**D.intr_kw(case.p["color"]))
    g.setExtrinsics(case.p["rotation"], case.p["translation"])
    g.setReferenceCrop(True)
    out = g.compute(D.depth_view(case), D.color_view(case))
    assert (out.width, out.height, out.is_dense) == (7, 4, True)
    same_bytes(out.points, D.reference("reference_13x7")[0])
