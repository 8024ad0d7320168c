"""Numpy reference of the edge extractor: pcl::Edge::detectEdgeCanny (thresholds 40 / 100) on the gray image (r + g + b) // 3 of an
organized cloud, as include/rsreg.h ("edge features") and the header comment of csrc/edges.hip state it -- written from that
description, independent of oracle/edge_oracle.c and of the kernels, and returning every stage.

  gray    float((r + g + b) // 3), the colour word at byte 16 of a record read as b g r a
  sm      3x3 Gaussian, sigma 1: k = float(exp(-(i^2 + j^2) / 2)) (exp in double, rounded once), normalised by its float sum
  gx, gy  Sobel x / y of sm
          (all three: correlation, borders clamped stage by stage, one float sum over kernel rows then columns, float32
          operations one at a time)
  mag     sqrtf(gx * gx + gy * gy)
  angle   float(atan2(double gy, double gx)) * 57.29578f
  dir     0 / 1 / 2 / 3 = 0 / 45 / 90 / 135 degrees, the class tests written out; 255 = none of them
  mx      interior pixels only: mag if !(mag < 40) and mag >= both neighbours along the direction, else 0
  root    8-connected components of mx != 0 (the smallest pixel index of a pixel's component, -1 where mx == 0)
  keep    the pixels of the components that hold a pixel with !(mx < 100)
  indices keep's pixel indices, ascending
"""
import types

import numpy as np
from scipy import ndimage

F = np.float32
T_LOW, T_HIGH = F(40.0), F(100.0)
RAD2DEG = F(57.29578)
SOBEL_X = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], F)
SOBEL_Y = np.array([[-1, -2, -1], [0, 0, 0], [1, 2, 1]], F)
# the two neighbours along the gradient, (di, dj) of the first; the second is its mirror image
NEIGHBOUR = {0: (0, -1), 1: (-1, -1), 2: (-1, 0), 3: (-1, 1)}
CLASS_BOUNDARIES = (22.5, 67.5, 112.5, 157.5, -22.5, -67.5, -112.5, -157.5)


def gaussian_kernel():
    k = np.zeros((3, 3), F)
    total = F(0.0)
    for i in range(3):
        for j in range(3):
            k[i, j] = F(np.exp(-np.float64((i - 1) ** 2 + (j - 1) ** 2) / 2.0))
            total = F(total + k[i, j])
    return (k / total).astype(F)


def correlate3(img, k):
    """out[i, j] = sum over kr, kc (in that order, one float32 product and one float32 sum at a time) of k[kr, kc] * img at the
    clamped coordinate"""
    h, w = img.shape
    pad = np.pad(img.astype(F), 1, mode="edge")       # (a halo of one pixel: the value at the clamped coordinate)
    s = np.zeros((h, w), F)
    for kr in range(3):
        for kc in range(3):
            s = (s + (F(k[kr, kc]) * pad[kr:kr + h, kc:kc + w]).astype(F)).astype(F)
    return s


def gray_of(rgba, w, h):
    c = np.asarray(rgba, np.uint32).reshape(h, w)
    b, g, r = c & 255, (c >> 8) & 255, (c >> 16) & 255
    return ((r.astype(np.int64) + g + b) // 3).astype(F)


def classify(angle):
    a = angle
    d = np.full(a.shape, 255, np.uint8)
    c0 = ((a <= F(22.5)) & (a >= F(-22.5))) | (a >= F(157.5)) | (a <= F(-157.5))
    c1 = ((a > F(22.5)) & (a < F(67.5))) | ((a < F(-112.5)) & (a > F(-157.5)))
    c2 = ((a >= F(67.5)) & (a <= F(112.5))) | ((a <= F(-67.5)) & (a >= F(-112.5)))
    c3 = ((a > F(112.5)) & (a < F(157.5))) | ((a < F(-22.5)) & (a > F(-67.5)))
    d[c3] = 3
    d[c2] = 2
    d[c1] = 1
    d[c0] = 0          # (the tests exclude each other for every angle; written in the order of the if / else if chain all the same)
    return d


def canny(rgba, w, h):
    """every stage of the extractor for the colour words `rgba` (w * h of them, row-major) -> a namespace of (h, w) arrays and
    `indices`"""
    w, h = int(w), int(h)
    gray = gray_of(rgba, w, h)
    sm = correlate3(gray, gaussian_kernel())
    gx, gy = correlate3(sm, SOBEL_X), correlate3(sm, SOBEL_Y)
    mag = np.sqrt(((gx * gx).astype(F) + (gy * gy).astype(F)).astype(F)).astype(F)
    angle = (np.arctan2(gy.astype(np.float64), gx.astype(np.float64)).astype(F) * RAD2DEG).astype(F)
    dr = classify(angle)
    mx = np.zeros((h, w), F)
    pm = np.pad(mag, 1, mode="constant")                # (never read: only interior pixels are suppressed)
    interior = np.zeros((h, w), bool)
    interior[1:h - 1, 1:w - 1] = True
    for c, (di, dj) in NEIGHBOUR.items():
        a = pm[1 + di:1 + di + h, 1 + dj:1 + dj + w]
        b = pm[1 - di:1 - di + h, 1 - dj:1 - dj + w]
        ok = interior & (dr == c) & ~(mag < T_LOW) & (mag >= a) & (mag >= b)
        mx[ok] = mag[ok]
    lab, n_comp = ndimage.label(mx != 0, structure=np.ones((3, 3), int))
    root = np.full((h, w), -1, np.int64)
    keep = np.zeros((h, w), bool)
    if n_comp:
        flat = lab.reshape(-1)
        first = np.full(n_comp + 1, w * h, np.int64)
        np.minimum.at(first, flat, np.arange(w * h))
        root = np.where(lab > 0, first[lab], -1)
        strong = np.zeros(n_comp + 1, bool)
        strong[np.unique(lab[(mx != 0) & ~(mx < T_HIGH)])] = True
        strong[0] = False
        keep = strong[lab]
    indices = np.flatnonzero(keep.reshape(-1)).astype(np.int32)
    return types.SimpleNamespace(w=w, h=h, gray=gray, sm=sm, gx=gx, gy=gy, mag=mag, angle=angle, dir=dr, mx=mx, root=root, keep=keep,
                                 indices=indices)


def edge_indices(points, w, h):
    return canny(points["rgba"], w, h).indices
