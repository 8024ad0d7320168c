"""The frames the capture step (depth + colour image -> organized cloud) is tested on, and the runners of its entry points.
Each case is small; tests/test_depthcloud_cpu.py shows from the numpy reference alone that a case holds what it is here for.

A case: depth and colour image in row-padded byte buffers (the padding is random, never zero), their strides, and the parameter
dict of tests/depthcloud_ref.py.  reference(name) is computed once and shared, read-only."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

import depthcloud_ref as R

F = np.float32
Case = namedtuple("Case", "dbuf dstride cbuf cstride p")


def frame(rng, dw, dh, cw, ch, bpp=3, dpad=0, cpad=0, depth=None, zeros=0.15):
    """(depth buffer, stride, colour buffer, stride): rows of random content with `dpad` / `cpad` bytes of random padding each"""
    dstride, cstride = 2 * dw + dpad, bpp * cw + cpad
    dbuf = rng.integers(1, 256, (dh, dstride), dtype=np.uint8)
    if depth is None:
        depth = rng.integers(300, 5000, (dh, dw)).astype(np.uint16)
        depth[rng.random((dh, dw)) < zeros] = 0
    dbuf[:, : 2 * dw] = np.ascontiguousarray(depth.astype("<u2")).view(np.uint8).reshape(dh, 2 * dw)
    cbuf = rng.integers(1, 256, (ch, cstride), dtype=np.uint8)
    return dbuf, dstride, cbuf, cstride


def depth_view(case):
    h, w = case.p["depth"]["height"], case.p["depth"]["width"]
    return np.ascontiguousarray(case.dbuf[:, : 2 * w]).view("<u2").reshape(h, w)


def color_view(case):
    h, w, bpp = case.p["color"]["height"], case.p["color"]["width"], case.p["bpp"]
    return np.ascontiguousarray(case.cbuf[:, : bpp * w]).reshape(h, w, bpp)


def rot(ax, ay, az):
    """column-major 3 x 3 of Rz Ry Rx, float32"""
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    m = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return [F(v) for v in m.T.reshape(-1)]


DEPTH_K = (0.12, -0.31, 0.0021, -0.0013, 0.094)      # five non-zero coefficients either side
COLOR_K = (-0.055, 0.067, 0.0009, -0.0007, -0.021)
Q2_DEPTH = 2000                                       # the raw depth whose z the q2 == 0 case's translation cancels


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261018)
    c = {}
    # the smallest image, a camera that maps pixel (c, r) to the ray (c, r, 1): one wave with 29 idle lanes
    c["tiny_7x5_identity"] = Case(*frame(rng, 7, 5, 7, 5), R.params(7, 5, color=R.intrinsics(7, 5, 0, 0, 1, 1), depth=R.intrinsics(7, 5, 0, 0, 1, 1)))
    # several workgroups and a ragged tail; a camera like a D435's, the colour sensor 15 mm to the side
    c["ragged_67x131"] = Case(*frame(rng, 67, 131, 67, 131),
                              R.params(67, 131, depth=R.intrinsics(67, 131, 33.1, 64.7, 61.3, 61.9), color=R.intrinsics(67, 131, 32.4, 66.2, 60.2, 60.4),
                                       rotation=rot(0.004, -0.002, 0.003), translation=[F(0.015), F(0.0003), F(-0.0002)]))
    # every raw depth value once; the only zero sits under a ray with negative x and y
    every = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    for tag, scale in (("001", 0.001), ("odd", 0.0012345679)):
        c["all_u16_scale_" + tag] = Case(*frame(rng, 256, 256, 256, 256, depth=every),
                                         R.params(256, 256, depth=R.intrinsics(256, 256, 127.5, 127.5, 210.0, 211.0),
                                                  color=R.intrinsics(256, 256, 126.0, 129.0, 205.0, 206.0), depth_scale=F(scale),
                                                  translation=[F(0.02), F(0), F(0)]))
    # padded rows, both pixel sizes, both channel orders
    for bpp in (3, 4):
        for bgr in (1, 0):
            c["padded_bpp%d_%s" % (bpp, "bgr" if bgr else "rgb")] = Case(*frame(rng, 16, 12, 16, 12, bpp=bpp, dpad=6, cpad=5),
                                                                         R.params(16, 12, bpp=bpp, bgr=bgr))
    # a colour image of another size (the reference pairs 1280 x 720 with the depth size)
    c["color_32x18_depth_16x12"] = Case(*frame(rng, 16, 12, 32, 18), R.params(16, 12, color=R.intrinsics(32, 18, 16.3, 8.8, 29.0, 29.5),
                                                                               translation=[F(0.01), F(-0.004), F(0.001)]))
    # a wide depth camera against a narrow colour camera, rotated: texture coordinates leave the colour image on all four sides
    c["extrinsics_clamp"] = Case(*frame(rng, 24, 20, 24, 20, zeros=0.05),
                                 R.params(24, 20, depth=R.intrinsics(24, 20, 11.5, 9.5, 10.0, 10.0), color=R.intrinsics(24, 20, 12.0, 10.0, 40.0, 40.0),
                                          rotation=rot(0.02, -0.03, 0.05), translation=[F(0.03), F(-0.02), F(0.01)]))
    # everything a power of two: u * width + .5f is exactly c + 0.5
    c["exact_half"] = Case(*frame(rng, 8, 4, 8, 4, depth=np.full((4, 8), 8, np.uint16)),
                           R.params(8, 4, depth=R.intrinsics(8, 4, 0, 0, 1, 1), color=R.intrinsics(8, 4, 0, 0, 1, 1), depth_scale=F(0.25)))
    # q2 == 0: the translation takes the z of one depth value away; columns left of, on and right of ppx -> -inf, NaN, +inf
    dq = rng.integers(300, 5000, (6, 9)).astype(np.uint16)
    dq[1::2, :] = Q2_DEPTH
    c["q2_zero"] = Case(*frame(rng, 9, 6, 9, 6, depth=dq),
                        R.params(9, 6, depth=R.intrinsics(9, 6, 4.0, 3.0, 8.0, 8.0), color=R.intrinsics(9, 6, 4.5, 3.0, 8.0, 8.0),
                                 translation=[F(0), F(0), -(F(0.001) * F(Q2_DEPTH))]))
    # both distortion forms, five non-zero coefficients each
    c["distortion_both"] = Case(*frame(rng, 40, 30, 40, 30),
                                R.params(40, 30, depth=R.intrinsics(40, 30, 19.3, 15.2, 28.0, 28.5, R.INVERSE_BROWN_CONRADY, DEPTH_K),
                                         color=R.intrinsics(40, 30, 20.1, 14.6, 27.0, 27.2, R.MODIFIED_BROWN_CONRADY, COLOR_K),
                                         rotation=rot(-0.003, 0.004, 0.002), translation=[F(0.015), F(0), F(0)]))
    # models of the other side or not built, all coefficients zero (one of them -0): accepted, act as none
    c["foreign_models_zero_coeffs"] = Case(*frame(rng, 16, 12, 16, 12),
                                           R.params(16, 12, depth=R.intrinsics(16, 12, model=R.BROWN_CONRADY), color=R.intrinsics(16, 12, model=R.INVERSE_BROWN_CONRADY,
                                                                                                                            coeffs=(0, -0.0, 0, 0, 0))))
    # ... and a model that is "none" ignores its coefficients
    c["none_ignores_coeffs"] = Case(*c["foreign_models_zero_coeffs"][:4], R.params(16, 12, depth=R.intrinsics(16, 12, coeffs=DEPTH_K), color=R.intrinsics(16, 12, coeffs=COLOR_K)))
    # the reference's three-fifths crop: cols 2 .. 8 into a cloud 7 wide; the real quirk (507 columns, width 508); an exact fit
    for w, h in ((13, 7), (848, 480), (640, 480)):
        c["reference_%dx%d" % (w, h)] = Case(*frame(rng, w, h, w, h),
                                            R.params_reference(w, h, depth=R.intrinsics(w, h, fx=0.72 * w, fy=0.72 * w), color=R.intrinsics(w, h, fx=0.7 * w, fy=0.7 * w),
                                                               translation=[F(0.015), F(0), F(0)]))
    # an empty window: every record the default
    c["empty_window"] = Case(*frame(rng, 4, 3, 4, 3), R.params(4, 3, r0=2, r1=2))
    for case in c.values():
        case.dbuf.flags.writeable = case.cbuf.flags.writeable = False
    return c


def invalid():
    """name -> (params dict, depth stride, colour stride) the contract refuses, one branch each; the images are tiny_7x5's"""
    ok = lambda **kw: R.params(7, 5, **kw)
    big = R.intrinsics(46341, 46341)
    return {
        "zero_depth_width": (ok(depth=R.intrinsics(0, 5)), 14, 21),
        "zero_depth_height": (ok(depth=R.intrinsics(7, 0)), 14, 21),
        "zero_color_width": (ok(color=R.intrinsics(0, 5)), 14, 21),
        "zero_color_height": (ok(color=R.intrinsics(7, 0)), 14, 21),
        "zero_out_width": (ok(out_width=0), 14, 21),
        "zero_out_height": (ok(out_height=0), 14, 21),
        "bpp_2": (ok(bpp=2), 14, 21),
        "bpp_5": (ok(bpp=5), 14, 35),
        "depth_stride_short": (ok(), 12, 21),
        "depth_stride_odd": (ok(), 15, 21),
        "color_stride_short": (ok(), 14, 20),
        "color_stride_short_bpp4": (ok(bpp=4), 14, 27),
        "window_r0_negative": (ok(r0=-1), 14, 21),
        "window_r1_past": (ok(r1=6), 14, 21),
        "window_rows_reversed": (ok(r0=3, r1=2), 14, 21),
        "window_c0_negative": (ok(c0=-1), 14, 21),
        "window_c1_past": (ok(c1=8), 14, 21),
        "window_cols_reversed": (ok(c0=5, c1=4), 14, 21),
        "window_larger_than_cloud": (ok(out_width=17, out_height=2), 14, 21),
        "too_many_records": (R.params(46341, 46341, depth=big, color=R.intrinsics(7, 5), r1=0, c1=0), 2 * 46341, 21),
        "depth_model_modified_nonzero": (ok(depth=R.intrinsics(7, 5, model=R.MODIFIED_BROWN_CONRADY, coeffs=(0, 0, 0, 0, 1e-9))), 14, 21),
        "depth_model_brown_conrady_nonzero": (ok(depth=R.intrinsics(7, 5, model=R.BROWN_CONRADY, coeffs=(0.1, 0, 0, 0, 0))), 14, 21),
        "depth_model_nan_coeff": (ok(depth=R.intrinsics(7, 5, model=R.FTHETA, coeffs=(0, np.nan, 0, 0, 0))), 14, 21),
        "color_model_inverse_nonzero": (ok(color=R.intrinsics(7, 5, model=R.INVERSE_BROWN_CONRADY, coeffs=(0, 0, 0.01, 0, 0))), 14, 21),
        "color_model_kannala_nonzero": (ok(color=R.intrinsics(7, 5, model=R.KANNALA_BRANDT4, coeffs=(0, 0, 0, 0.2, 0))), 14, 21),
        "depth_model_unknown": (ok(depth=R.intrinsics(7, 5, model=6)), 14, 21),
        "color_model_negative": (ok(color=R.intrinsics(7, 5, model=-1)), 14, 21),
    }


@functools.lru_cache(maxsize=None)
def reference(name, **variant):
    case = cases()[name]
    out, w, h, dense, dbg = R.depth_to_cloud(depth_view(case), color_view(case), case.p, **variant)
    out.flags.writeable = False
    for a in dbg.values():
        a.flags.writeable = False
    return out, (len(out), 32, w, h, dense), dbg


def intr_kw(d):
    """an intrinsics dict -> the keyword arguments of api.DepthToCloud.setDepthIntrinsics / setColorIntrinsics"""
    return {k: (d[k] if k in ("width", "height", "model") else [float(v) for v in d[k]] if k == "coeffs" else float(d[k])) for k in d}


def frame_images(cloud):
    """an organized synth.render_frame cloud -> (depth (h, w) uint16 in mm, colour (h, w, 3) uint8 in b, g, r order, the
    parameter dict of the pinhole that rendered it): what a camera would have delivered"""
    w, h = cloud.width, cloud.height
    depth = np.rint(cloud.points["z"].astype(np.float64) * 1000.0).astype(np.uint16).reshape(h, w)
    rgba = cloud.points["rgba"].reshape(h, w)
    color = np.stack([rgba & 0xff, (rgba >> 8) & 0xff, (rgba >> 16) & 0xff], axis=2).astype(np.uint8)
    f = 385.0 * (w / 640.0)
    cam = R.intrinsics(w, h, w / 2.0, h / 2.0, f, f)
    return depth, color, R.params(w, h, depth=cam, color=dict(cam))


def c_params(lib, p):
    """the parameter dict -> rsreg_depth_params"""
    q = lib.DepthParams()
    for side in ("depth", "color"):
        s, d = getattr(q, side), p[side]
        s.width, s.height, s.model = d["width"], d["height"], d["model"]
        s.ppx, s.ppy, s.fx, s.fy = [float(d[k]) for k in ("ppx", "ppy", "fx", "fy")]
        for i in range(5):
            s.coeffs[i] = float(d["coeffs"][i])
    for i in range(9):
        q.rotation[i] = float(p["rotation"][i])
    for i in range(3):
        q.translation[i] = float(p["translation"][i])
    q.depth_scale, q.color_bytes_per_pixel, q.color_bgr = float(p["depth_scale"]), p["bpp"], p["bgr"]
    q.r0, q.r1, q.c0, q.c1 = p["r0"], p["r1"], p["c0"], p["c1"]
    q.out_width, q.out_height, q.is_dense = p["out_width"], p["out_height"], p["is_dense"]
    return q


def params_dict(q):
    """rsreg_depth_params -> the parameter dict (what the C helpers filled in)"""
    side = lambda s: {"width": s.width, "height": s.height, "ppx": F(s.ppx), "ppy": F(s.ppy), "fx": F(s.fx), "fy": F(s.fy), "model": s.model,
                      "coeffs": [F(v) for v in s.coeffs]}
    return {"depth": side(q.depth), "color": side(q.color), "rotation": [F(v) for v in q.rotation], "translation": [F(v) for v in q.translation],
            "depth_scale": F(q.depth_scale), "bpp": q.color_bytes_per_pixel, "bgr": q.color_bgr, "r0": q.r0, "r1": q.r1, "c0": q.c0, "c1": q.c1,
            "out_width": q.out_width, "out_height": q.out_height, "is_dense": q.is_dense}


def run_host(lib, case):
    """rsreg_depth_to_cloud -> (records, (n, 32, width, height, is_dense))"""
    n = case.p["out_width"] * case.p["out_height"]
    out = np.full(n, 0x5a, np.uint8).repeat(32).view(R.POINT)      # (every byte has to be written)
    w, h, dense = C.c_uint32(0), C.c_uint32(0), C.c_int(-1)
    q = c_params(lib, case.p)
    lib.check(lib.lib().rsreg_depth_to_cloud(case.dbuf.ctypes.data, case.dstride, case.cbuf.ctypes.data, case.cstride, C.byref(q), out.ctypes.data, n,
                                             C.byref(w), C.byref(h), C.byref(dense)))
    return out, (n, 32, w.value, h.value, dense.value)


class Handle:
    """a device cloud through the C ABI"""

    def __init__(self, lib, ctx):
        self.lib, self.ctx, self.h = lib, ctx, C.c_void_p()
        lib.check(lib.lib().rsreg_cloud_create(ctx.h, C.byref(self.h)), ctx.h)

    def info(self):
        n, s, w, h, d = C.c_size_t(0), C.c_size_t(0), C.c_uint32(0), C.c_uint32(0), C.c_int(0)
        self.lib.check(self.lib.lib().rsreg_cloud_info(self.h, C.byref(n), C.byref(s), C.byref(w), C.byref(h), C.byref(d)), self.ctx.h)
        return n.value, s.value, w.value, h.value, d.value

    def version(self):
        i, v = C.c_uint64(0), C.c_uint64(0)
        self.lib.check(self.lib.lib().rsreg_cloud_version(self.h, C.byref(i), C.byref(v)))
        return v.value

    def download(self):
        n = self.info()[0]
        out = np.zeros(n, R.POINT)
        self.lib.check(self.lib.lib().rsreg_cloud_download(self.h, out.ctypes.data, n), self.ctx.h)
        return out

    def close(self):
        if self.h:
            self.lib.lib().rsreg_cloud_destroy(self.h)
            self.h = None


def device_bytes(lib, ctx, buf):
    """the bytes of `buf` in HBM, through the library's own upload (as 16-byte records of a cloud that is kept alive by the
    caller): (Handle, device address)"""
    raw = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    padded = np.zeros((len(raw) + 15) // 16 * 16, np.uint8)
    padded[: len(raw)] = raw
    h = Handle(lib, ctx)
    lib.check(lib.lib().rsreg_cloud_upload(h.h, padded.ctypes.data, len(padded) // 16, 16, len(padded) // 16, 1, 0), ctx.h)
    return h, int(lib.lib().rsreg_cloud_device_ptr(h.h))


def run_gpu(lib, ctx, case, out, device=False):
    """rsreg_cloud_from_depth (host images) or, device=True, rsreg_cloud_from_depth_device (the images put into HBM first) into
    the Handle `out` -> (records, meta, version before, version after)"""
    q = c_params(lib, case.p)
    before = out.version()
    if device:
        (dh, d_ptr), (ch, c_ptr) = device_bytes(lib, ctx, case.dbuf), device_bytes(lib, ctx, case.cbuf)
        lib.check(lib.lib().rsreg_cloud_from_depth_device(ctx.h, d_ptr, case.dstride, c_ptr, case.cstride, C.byref(q), out.h), ctx.h)
        lib.check(lib.lib().rsreg_ctx_synchronize(ctx.h), ctx.h)      # (the images stay alive until here)
        dh.close()
        ch.close()
    else:
        lib.check(lib.lib().rsreg_cloud_from_depth(ctx.h, case.dbuf.ctypes.data, case.dstride, case.cbuf.ctypes.data, case.cstride, C.byref(q), out.h),
                  ctx.h)
    return out.download(), out.info(), before, out.version()
