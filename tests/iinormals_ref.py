"""pcl::IntegralImageNormalEstimation (AVERAGE_3D_GRADIENT, border policy IGNORE, no depth-dependent smoothing) as
include/rsreg.h states it for rsreg_cloud_integral_normals, in numpy: the reference of tests/test_iinormals_cpu.py and
tests/test_iinormals_gpu.py.

(a) - (d) are float32, operation by operation.  The two chamfer passes of the distance map are the sequential loops over PCL's
flat index, quirks included.  The window sums are float64, taken from a summed-area table: numpy's cumsum by default, or
(table="recurrence") filled as PCL fills it, S[r][c] = S[r-1][c] + S[r][c-1] - S[r-1][c-1] + x.
"""
import struct
from types import SimpleNamespace

import numpy as np

F32 = np.float32
QNAN = 0x7fc00000
_F14, _F10 = float(F32(1.4)), 1.0


def _f32(x):
    """A Python float rounded to float32 (the sum of two float32 values in double is exact: one rounding, as in float32)."""
    return struct.unpack("f", struct.pack("f", x))[0]


def depth_change_map(z, factor):
    """M (h, w) bool: False where the pixel takes part in a depth change."""
    z = np.asarray(z, F32)
    h, w = z.shape
    M = np.ones((h, w), bool)
    if h < 2 or w < 2:
        return M
    f = F32(factor)
    c = z[:-1, :-1]
    with np.errstate(invalid="ignore", over="ignore"):
        t = (f * (np.abs(c) + F32(1.0))) * F32(2.0)
        assert t.dtype == F32
        for nb, (dr, dc) in ((z[:-1, 1:], (0, 1)), (z[1:, :-1], (1, 0))):
            bad = (np.abs(c - nb) > t) | ~np.isfinite(c) | ~np.isfinite(nb)
            M[:-1, :-1][bad] = False
            M[dr:h - 1 + dr, dc:w - 1 + dc][bad] = False
    return M


def distance_map(M):
    """D (h, w) float32 after the forward and the backward pass, sequential, PCL's flat indexing."""
    M = np.asarray(M, bool)
    h, w = M.shape
    big = float(F32(w + h))
    D = [0.0 if not m else big for m in M.reshape(-1)]
    for r in range(1, h):
        for c in range(1, w):
            i = r * w + c
            m = min(min(_f32(D[i - w - 1] + _F14), _f32(D[i - w] + _F10)), min(_f32(D[i - 1] + _F10), _f32(D[i - w + 1] + _F14)))
            if m < D[i]:
                D[i] = m
    for r in range(h - 2, -1, -1):
        for c in range(w - 2, -1, -1):
            i = r * w + c
            m = min(min(_f32(D[i + w - 1] + _F14), _f32(D[i + 1] + _F10)), min(_f32(D[i + w] + _F10), _f32(D[i + w + 1] + _F14)))
            if m < D[i]:
                D[i] = m
    return np.array(D, F32).reshape(h, w)


def rect_map(z, D, smoothing):
    """R (h, w) uint8: the window size, 0 = no window."""
    z = np.asarray(z, F32)
    h, w = z.shape
    B = int(F32(smoothing))
    R = np.zeros((h, w), np.uint8)
    if w <= 2 * B or h <= 2 * B:
        return R
    sm = np.minimum(D, F32(smoothing))
    ok = np.isfinite(z) & (sm > F32(2.0))
    inner = np.zeros((h, w), bool)
    inner[B:h - B, B:w - B] = True
    ok &= inner
    R[ok] = sm[ok].astype(np.int32).astype(np.uint8)
    return R


def differences(P):
    """DX, DY (h, w, 3) float32 and which of their elements are finite."""
    P = np.asarray(P, F32)
    h, w, _ = P.shape
    DX, DY = np.zeros((h, w, 3), F32), np.zeros((h, w, 3), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        if h > 2 and w > 2:
            DX[1:-1, 1:-1] = P[1:-1, 2:] - P[1:-1, :-2]
            DY[1:-1, 1:-1] = P[2:, 1:-1] - P[:-2, 1:-1]
        fx = np.isfinite((DX[..., 0] + DX[..., 1]) + DX[..., 2])
        fy = np.isfinite((DY[..., 0] + DY[..., 1]) + DY[..., 2])
    return DX, DY, fx, fy


def _table(x, order):
    """The summed-area table of x (h, w, k) float64 with a row and a column of zeros in front."""
    h, w, k = x.shape
    S = np.zeros((h + 1, w + 1, k), np.float64)
    if order == "cumsum":
        S[1:, 1:] = np.cumsum(np.cumsum(x, axis=0), axis=1)
    else:
        assert order == "recurrence"
        for r in range(1, h + 1):
            for c in range(1, w + 1):
                S[r, c] = S[r - 1, c] + S[r, c - 1] - S[r - 1, c - 1] + x[r - 1, c - 1]
    return S


def _window(S, r0, c0, R):
    r1, c1 = r0 + R, c0 + R
    return S[r1, c1] + S[r0, c0] - S[r0, c1] - S[r1, c0]


def normals(P, factor=0.02, smoothing=10.0, viewpoint=(0.0, 0.0, 0.0), table="cumsum"):
    """P: (h, w, 3) float32.  Returns records (h * w, 8) uint32 -- the output cloud's words -- rect (h * w,) uint8, D, and per
    record has_normal, l, |gx|^2, |gy|^2 (float64; 0 where there is no window)."""
    P = np.asarray(P, F32)
    h, w, _ = P.shape
    z = P[..., 2]
    D = distance_map(depth_change_map(z, factor))
    R = rect_map(z, D, smoothing)
    DX, DY, fx, fy = differences(P)
    x = np.concatenate([np.where(fx[..., None], DX, 0).astype(np.float64), np.where(fy[..., None], DY, 0).astype(np.float64),
                        fx[..., None].astype(np.float64), fy[..., None].astype(np.float64)], axis=2)
    S = _table(x, table)
    rr, cc = np.nonzero(R)
    Rw = R[rr, cc].astype(np.int64)
    win = _window(S, rr - Rw // 2, cc - Rw // 2, Rw)
    gx, gy, cnt_x, cnt_y = win[:, 0:3], win[:, 3:6], win[:, 6], win[:, 7]
    n = np.stack([gy[:, 1] * gx[:, 2] - gy[:, 2] * gx[:, 1], gy[:, 2] * gx[:, 0] - gy[:, 0] * gx[:, 2], gy[:, 0] * gx[:, 1] - gy[:, 1] * gx[:, 0]], axis=1)
    l = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    has = (cnt_x != 0) & (cnt_y != 0) & (l != 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nf = (n / np.sqrt(l)[:, None]).astype(F32)
        v = np.asarray(viewpoint, F32)[None, :] - P[rr, cc]
        cos = (v[:, 0] * nf[:, 0] + v[:, 1] * nf[:, 1]) + v[:, 2] * nf[:, 2]
        assert cos.dtype == F32
        nf = np.where((cos < 0)[:, None], -nf, nf)
    rec = np.zeros((h * w, 8), np.uint32)
    rec[:, [0, 1, 2, 4]] = QNAN
    at = (rr * w + cc)[has]
    rec[at, 0:3] = nf[has].view(np.uint32)
    flat = lambda a: _scatter(h * w, rr * w + cc, a)
    return SimpleNamespace(records=rec, rect=R.reshape(-1), D=D, has_normal=flat(has).astype(bool), l=flat(l),
                           gx2=flat((gx * gx).sum(axis=1)), gy2=flat((gy * gy).sum(axis=1)))


def _scatter(n, at, values):
    out = np.zeros(n, np.float64)
    out[at] = values
    return out


def normal_vectors(records):
    """(n, 3) float32 view of the normals in `records`."""
    return np.ascontiguousarray(records[:, 0:3]).view(F32)
