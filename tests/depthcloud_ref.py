"""The capture step -- a depth image and a colour image -> an organized PointXYZRGB cloud -- in numpy, written from the
contract in include/rsreg.h ("capture") and from nothing else: independent of csrc/depth_host.cpp and of
csrc/depthcloud_kernels.hpp.

Every operation is a float32 numpy operation on float32 arrays (one IEEE rounding each, no multiply-add), in the order the
contract writes them.  Parameters are a plain dict (params()), not the ctypes struct.
"""
import numpy as np

F = np.float32
NONE, MODIFIED_BROWN_CONRADY, INVERSE_BROWN_CONRADY, FTHETA, BROWN_CONRADY, KANNALA_BRANDT4 = range(6)

POINT = np.dtype({"names": ["x", "y", "z", "w", "rgba"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u4"], "offsets": [0, 4, 8, 12, 16],
                  "itemsize": 32})


def intrinsics(width, height, ppx=None, ppy=None, fx=None, fy=None, model=NONE, coeffs=(0, 0, 0, 0, 0)):
    return {"width": int(width), "height": int(height), "ppx": F(width / 2 if ppx is None else ppx), "ppy": F(height / 2 if ppy is None else ppy),
            "fx": F(width if fx is None else fx), "fy": F(width if fy is None else fy), "model": int(model),
            "coeffs": [F(c) for c in coeffs]}


def params(w, h, color=None, **kw):
    """rsreg_depth_params_default(w, h) as a dict: the whole frame, the cloud w x h, is_dense 0"""
    p = {"depth": intrinsics(w, h), "color": color or intrinsics(w, h),
         "rotation": [F(v) for v in (1, 0, 0, 0, 1, 0, 0, 0, 1)], "translation": [F(0)] * 3, "depth_scale": F(0.001),
         "bpp": 3, "bgr": 1, "r0": 0, "r1": h, "c0": 0, "c1": w, "out_width": w, "out_height": h, "is_dense": 0}
    p.update(kw)
    return p


def params_reference(w, h, **kw):
    """rsreg_depth_params_reference(w, h): the three-fifths centre crop, C integer division (w, h >= 0: // is C's /)"""
    return params(w, h, **dict({"r0": h // 5, "r1": h // 5 * 4, "c0": w // 5, "c1": w // 5 * 4, "out_width": w * 3 // 5, "out_height": h * 3 // 5,
                                "is_dense": 1}, **kw))


def model_use(intr, own):
    """0: acts as none, 1: the side's own form applies, None: refused"""
    if not 0 <= intr["model"] <= 5:
        return None
    if intr["model"] == NONE:
        return 0
    if intr["model"] == own:
        return 1
    return 0 if all(F(c) == F(0) for c in intr["coeffs"]) else None


def refused(p, depth_stride, color_stride):
    """True where the contract says RSREG_ERR_INVALID_ARG"""
    d, c = p["depth"], p["color"]
    if min(d["width"], d["height"], c["width"], c["height"], p["out_width"], p["out_height"]) <= 0:
        return True
    if p["bpp"] not in (3, 4):
        return True
    if depth_stride < 2 * d["width"] or depth_stride % 2 or color_stride < p["bpp"] * c["width"]:
        return True
    if not (0 <= p["r0"] <= p["r1"] <= d["height"] and 0 <= p["c0"] <= p["c1"] <= d["width"]):
        return True
    n = p["out_width"] * p["out_height"]
    if (p["r1"] - p["r0"]) * (p["c1"] - p["c0"]) > n or n > 2 ** 31 - 16:
        return True
    return model_use(d, INVERSE_BROWN_CONRADY) is None or model_use(c, MODIFIED_BROWN_CONRADY) is None


def to_int(t):
    """C's (int)t for a float32 array; INT_MIN where C leaves it undefined (NaN, outside [-2^31, 2^31)): the x86 rule"""
    t = np.asarray(t, F)
    ok = (t >= F(-2147483648.0)) & (t < F(2147483648.0))
    out = np.full(t.shape, -2 ** 31, np.int64)
    out[ok] = np.trunc(t[ok]).astype(np.int64)
    return out


def _radial(k, r2):
    return F(1) + k[0] * r2 + k[1] * r2 * r2 + k[4] * r2 * r2 * r2


def depth_to_cloud(depth, color, p, swap_channels=False, no_half=False):
    """depth: (h, w) uint16 array; color: (h, w, bpp) uint8 array (views of padded buffers are fine: only pixels are indexed).
    Returns (records, width, height, is_dense, dbg); dbg holds intermediate arrays over the window's pixels, row-major:
    P (n, 3), u, v, tx, ty (the floats that are cast), ix, iy (the casts before the clamp), xi, yi."""
    d_in, c_in = p["depth"], p["color"]
    assert depth.shape == (d_in["height"], d_in["width"]) and depth.dtype == np.uint16
    assert color.shape == (c_in["height"], c_in["width"], p["bpp"]) and color.dtype == np.uint8
    n = p["out_width"] * p["out_height"]
    out = np.zeros(n, POINT)
    out["w"], out["rgba"] = F(1), 0xff000000
    rows, cols = np.arange(p["r0"], p["r1"]), np.arange(p["c0"], p["c1"])
    count = len(rows) * len(cols)
    dbg = {}
    if count:
        with np.errstate(all="ignore"):
            r, c = [a.reshape(-1) for a in np.meshgrid(rows, cols, indexing="ij")]
            d = depth[r, c]
            # (1) the vertex
            z = p["depth_scale"] * d.astype(F)
            x = (c.astype(F) - d_in["ppx"]) / d_in["fx"]
            y = (r.astype(F) - d_in["ppy"]) / d_in["fy"]
            if model_use(d_in, INVERSE_BROWN_CONRADY) == 1:
                k = d_in["coeffs"]
                r2 = x * x + y * y
                f = _radial(k, r2)
                ux = x * f + F(2) * k[2] * x * y + k[3] * (r2 + F(2) * x * x)
                uy = y * f + F(2) * k[3] * x * y + k[2] * (r2 + F(2) * y * y)
                x, y = ux, uy
            P = np.stack([z * x, z * y, z], axis=1)
            # (2) the texture coordinate
            R, t = p["rotation"], p["translation"]
            q = [R[0 + k] * P[:, 0] + R[3 + k] * P[:, 1] + R[6 + k] * P[:, 2] + t[k] for k in range(3)]
            tx, ty = q[0] / q[2], q[1] / q[2]
            if model_use(c_in, MODIFIED_BROWN_CONRADY) == 1:
                k = c_in["coeffs"]
                r2 = tx * tx + ty * ty
                f = _radial(k, r2)
                tx, ty = tx * f, ty * f
                dx = tx + F(2) * k[2] * tx * ty + k[3] * (r2 + F(2) * tx * tx)
                dy = ty + F(2) * k[3] * tx * ty + k[2] * (r2 + F(2) * ty * ty)
                tx, ty = dx, dy
            wf, hf = F(c_in["width"]), F(c_in["height"])
            u = (tx * c_in["fx"] + c_in["ppx"]) / wf
            v = (ty * c_in["fy"] + c_in["ppy"]) / hf
            zero = P[:, 2] == F(0)
            u, v = np.where(zero, F(0), u).astype(F), np.where(zero, F(0), v).astype(F)
            # (3) the colour
            half = F(0) if no_half else F(0.5)
            fx_, fy_ = u * wf + half, v * hf + half
            ix, iy = to_int(fx_), to_int(fy_)
            xi, yi = np.clip(ix, 0, c_in["width"] - 1), np.clip(iy, 0, c_in["height"] - 1)
            px = color[yi, xi].astype(np.uint32)
            first, last = px[:, 0], px[:, 2]
            red, blue = (last, first) if bool(p["bgr"]) != swap_channels else (first, last)
            for a in (P, u, v, fx_, fy_):
                assert a.dtype == F
        out["x"][:count], out["y"][:count], out["z"][:count] = P[:, 0], P[:, 1], P[:, 2]
        out["rgba"][:count] = np.uint32(0xff000000) | (red << 16) | (px[:, 1] << 8) | blue
        dbg = {"P": P, "u": u, "v": v, "tx": fx_, "ty": fy_, "ix": ix, "iy": iy, "xi": xi, "yi": yi, "q2": q[2], "d": d}
    return out, p["out_width"], p["out_height"], int(bool(p["is_dense"])), dbg
