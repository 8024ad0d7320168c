"""The images the edge-extractor tests run (CPU: the C oracle against tests/edges_ref.py, and the property each image is here for,
asserted on the reference's stages; GPU: csrc/edges.hip against both), the smallest at which each part of the extractor can go
wrong: tile seams and corners of the 32 x 32 tiles, images of a few pixels, both thresholds, equal neighbours in the
suppression, the direction-class boundaries, record strides and the blocks of the compaction.

A case is (records, width, height); build(name) makes one, indices(name) is the reference's answer, computed once."""
import functools
import math

import numpy as np

import edges_ref as R

TILE = 32                  # csrc/edges.hip: kCcTile
BLOCK = 4096               # csrc/compact.hpp: pixels per workgroup of the compaction


def _dtype(size):
    d = {"names": ["x", "y", "z", "w", "rgba"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u4"], "offsets": [0, 4, 8, 12, 16], "itemsize": size}
    if size > 32:          # (a 32-byte record is pcl::PointXYZRGB: twelve bytes of padding behind the colour)
        d["names"].append("extra")
        d["formats"].append(("<u4", (size - 20) // 4))
        d["offsets"].append(20)
    return np.dtype(d)


POINT20, POINT, POINT48 = _dtype(20), _dtype(32), _dtype(48)


def records(img, alpha=255, dtype=POINT):
    """(h, w) gray levels or (h, w, 3) r g b -> w * h records; the geometry names the pixel, so a record copied from the wrong
    pixel shows"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = np.repeat(img[:, :, None], 3, axis=2)
    assert img.min() >= 0 and img.max() <= 255
    h, w = img.shape[:2]
    c = img.astype(np.uint32).reshape(-1, 3)
    a = np.broadcast_to(np.asarray(alpha, np.uint32).reshape(-1), (w * h,)) if np.ndim(alpha) else np.full(w * h, alpha, np.uint32)
    pts = np.zeros(w * h, dtype)
    i = np.arange(w * h)
    pts["x"], pts["y"], pts["z"], pts["w"] = (i % w) * 0.01, (i // w) * 0.01, 1.0 + i * 1e-4, 1.0
    pts["rgba"] = (a << 24) | (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]
    if dtype.itemsize == 32:               # the twelve bytes behind the colour travel with the record: give them a value
        byte_rows(pts)[:, 20:] = ((i[:, None] * 12 + np.arange(12)) * 37 + 11) & 255
    return pts


def byte_rows(pts):
    """the records as rows of bytes (a view), padding included"""
    return pts.view(np.uint8).reshape(len(pts), pts.dtype.itemsize)


def clone(pts):
    """a copy byte for byte (numpy's own copies and fancy indexing go field by field and leave the padding undefined)"""
    out = np.zeros(len(pts), pts.dtype)
    byte_rows(out)[:] = byte_rows(pts)
    return out


def restride(pts, dtype):
    out = np.zeros(len(pts), dtype)
    for f in ("x", "y", "z", "w", "rgba"):
        out[f] = pts[f]
    if "extra" in dtype.names:
        out["extra"] = 0xdeadbeef          # a payload behind the colour: copied with the record, never read as colour
    elif dtype.itemsize == pts.dtype.itemsize:
        byte_rows(out)[:] = byte_rows(pts)
    return out


def noise(w, h, seed):
    """independent channels, uniform in 0..255: sums that are no multiples of 3"""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3))


# ---- shapes: a few pixels (one pixel clamped in several halos at once), one tile exactly, a last tile one pixel wide ----------
# seeds: the first of 0, 1, 2 ... at which the reference's edge points touch row 1, row h - 2, column 1 and column w - 2 and, where
# the last tile is partial and more than one pixel wide, lie inside it
SHAPES = {(3, 3): 0, (4, 3): 2, (3, 4): 2, (5, 5): 2, (6, 4): 4, (3, 40): 3, (40, 3): 14, (31, 31): 0, (32, 32): 0, (33, 33): 0, (34, 35): 0,
          (63, 33): 0, (64, 64): 0, (65, 34): 0, (97, 70): 0}


def step_3x3():
    return records(np.where(np.arange(9).reshape(3, 3) % 3 == 2, 255, 0)), 3, 3


# ---- seams: steps whose contrast fades gradually along the edge, from strong at one end to weak over the rest ------------------
SEAM_N = 100
# (thin: the step taken in two halves one pixel apart, so that one line of pixels holds the maximum, not two lines with equal
# magnitudes -- the points of a thin diagonal hang together through NW joins alone, those of a thin antidiagonal through NE joins)
# stairs: a thin edge that runs along a row (a column) for STAIR pixels and then moves to the next one: the two runs hang together
# through one diagonal join
SEAM_ORIENTATIONS = ("vertical", "horizontal", "diagonal", "antidiagonal", "zigzag", "thindiagonal", "thinantidiagonal",
                     "stairsdown", "stairsup", "stairsright", "stairsleft")
STAIR = 5
SEAM_OFFSETS = (0, 1, 31, 32, 33)
STRONG, WEAK, FADE = 120, 22, 4        # contrast at the strong end, over the weak part, and its decrease per pixel between them


def seam(orientation, strong_last, ox, oy, weak_only=False, n=SEAM_N):
    y, x = np.mgrid[0:n, 0:n]
    xs, ys = x - ox, y - oy
    half = None
    if orientation == "vertical":
        side, pos = xs >= TILE, ys
    elif orientation == "horizontal":
        side, pos = ys >= TILE, xs
    elif orientation == "diagonal":
        side, pos = xs - ys >= 0, (xs + ys) // 2
    elif orientation == "thindiagonal":
        side, half, pos = xs - ys >= 0, xs - ys >= 1, (xs + ys) // 2
    elif orientation in ("antidiagonal", "thinantidiagonal"):
        k = 2 * TILE - 1 + ox + oy
        side, pos = x + y >= k, y - max(0, k - (n - 1))
        half = x + y >= k + 1 if orientation == "thinantidiagonal" else None
    elif orientation in ("stairsdown", "stairsup"):
        line = TILE + (xs - TILE) // STAIR if orientation == "stairsdown" else TILE - 1 - (xs - TILE) // STAIR
        side, half, pos = ys >= line, ys >= line + 1, xs
    elif orientation in ("stairsright", "stairsleft"):
        line = TILE + (ys - TILE) // STAIR if orientation == "stairsright" else TILE - 1 - (ys - TILE) // STAIR
        side, half, pos = xs >= line, xs >= line + 1, ys
    else:
        side, pos = xs >= 40 + np.abs(ys % 16 - 8), ys
    edge = np.zeros((n, n), bool)                      # pixels with a neighbour on the other side
    edge[:, 1:] |= side[:, 1:] != side[:, :-1]
    edge[1:, :] |= side[1:, :] != side[:-1, :]
    t = (pos[edge & (pos >= 0)].max() - pos) if strong_last else pos
    contrast = np.where((pos >= 0) & (t >= 0), np.maximum(WEAK, STRONG - FADE * t), 0)
    if weak_only:
        contrast[contrast > WEAK] = 0
    if half is not None:
        return records(60 + (contrast // 2) * side + (contrast - contrast // 2) * half), n, n
    return records(60 + contrast * side), n, n


# ---- thresholds: a step of every height ----------------------------------------------------------------------------------------
THRESHOLD_ORIENTATIONS = ("vertical", "horizontal", "diagonal", "antidiagonal")


def step_side(orientation, w, h):
    y, x = np.mgrid[0:h, 0:w]
    return {"vertical": x >= w // 2, "horizontal": y >= h // 2, "diagonal": x - y >= (w - h) // 2, "antidiagonal": x + y >= (w + h) // 2 - 1}[orientation]


def threshold_step(orientation, delta):
    return records(delta * step_side(orientation, 12, 8)), 12, 8


def two_level(orientation, d_top, d_bottom, gap):
    """a step of height d_top over one of height d_bottom along the same line, `gap` flat rows (columns) between them"""
    side = step_side("vertical", 12, 20)
    y = np.mgrid[0:20, 0:12][0]
    img = np.where(y < 10 - gap // 2, d_top, np.where(y >= 10 + (gap + 1) // 2, d_bottom, 0)) * side
    if orientation == "horizontal":
        return records(img.T), 20, 12
    return records(img), 12, 20


# ---- magnitudes exactly on the thresholds: a step taken in two equal halves of k gray levels has magnitude 4 k, exactly or an ulp
# above it depending on the order of the sums -- 100 at k = 25, 40 at k = 10
def half_step_row(k, base, w=12):
    r = np.full(w, base)
    r[5:7] += k
    r[7:] += 2 * k
    return r


def exact_step(transposed=False):
    """gray 0 | 25 | 50: the largest magnitude is 100.0f exactly"""
    img = np.tile(half_step_row(25, 0), (8, 1))
    return (records(img.T), 8, 12) if transposed else (records(img), 12, 8)


EXACT_BASES, EXACT_VARIANTS = (0, 1, 7, 100), ("id", "lr", "ud", "T", "Tud")


def exact_fade(base, variant):
    """six rows of the half step at k = 25, one row each for k = 25 .. 11, eight rows at k = 10 (mirrored / transposed: the
    order of the float sums changes, and with it which of two neighbours is the larger by an ulp)"""
    img = np.array([half_step_row(k, base) for k in [25] * 6 + list(range(25, 10, -1)) + [10] * 8])
    img = {"id": img, "lr": img[:, ::-1], "ud": img[::-1], "T": img.T, "Tud": img.T[::-1]}[variant]
    return records(img), img.shape[1], img.shape[0]


# ---- suppression ties: bars and checkers two and three pixels wide ------------------------------------------------------------
def bars(kind, k, lo, hi, w=41, h=37):
    y, x = np.mgrid[0:h, 0:w]
    v = {"x": x // k, "y": y // k, "checker": x // k + y // k, "slant": (x + y) // k}[kind]
    return records(np.where(v % 2 == 1, hi, lo)), w, h


# ---- directions: planes and steps at given angles -------------------------------------------------------------------------------
def plane(a, b, n=20):
    y, x = np.mgrid[0:n, 0:n]
    g = a * x + b * y
    return records(np.rint(g - g.min()).astype(np.int64)), n, n


def angled_step(deg, n=24, contrast=120):
    y, x = np.mgrid[0:n, 0:n]
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return records(60 + contrast * (c * (x - n / 2 + 0.25) + s * (y - n / 2 + 0.25) >= 0)), n, n


PLANE_SLOPES = [(a, b) for a in (-6, -4, 0, 4, 6) for b in (-6, -4, 0, 4, 6) if a * a + b * b >= 32]


# ---- records and compaction ----------------------------------------------------------------------------------------------------
def scattered_non_finite(pts, seed=11):
    """NaN, +-inf and denormal bit patterns through x, y, z, w: the extractor reads the colour only"""
    rng = np.random.default_rng(seed)
    out = clone(pts)
    bits = np.array([0x7fc00000, 0xffc00001, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x7f800001], np.uint32)
    for f in ("x", "y", "z", "w"):
        where = rng.choice(len(out), len(out) // 7, replace=False)
        v = out[f].view(np.uint32).copy()
        v[where] = bits[rng.integers(0, len(bits), len(where))]
        out[f] = v.view(np.float32)
    return out


def one_channel(channel, w=40, h=30, seed=5):
    """contrast in one place only: r, b, the alpha byte, or x; everything else constant"""
    v = np.random.default_rng(seed).integers(0, 256, (h, w))
    v[:, w // 2:] //= 4
    img = np.full((h, w, 3), 100)
    if channel in ("r", "b"):
        img[:, :, 0 if channel == "r" else 2] = v
    pts = records(img, alpha=v.reshape(-1) if channel == "alpha" else 255)
    if channel == "x":
        pts["x"] = v.reshape(-1)
    return pts, w, h


COMPACT_W, COMPACT_H = 97, 130          # 12 610 pixels: three blocks of 4 096 and one of 322


def compaction(kind, seed=3):
    w, h = COMPACT_W, COMPACT_H
    img = np.full((h, w, 3), 128)
    nz = noise(w, h, seed)
    if kind in ("first", "first_and_last"):
        img[:36] = nz[:36]                                   # its edges end before pixel 40 * 97 = 3 880
    if kind in ("last", "first_and_last"):
        img[128:, 70:] = nz[128:, 70:]                       # its edges start behind pixel 126 * 97 + 68 = 12 290 > 3 * 4 096
    if kind == "dense":
        img = nz
    return records(img), w, h


# ---- the table -------------------------------------------------------------------------------------------------------------------
def _cases():
    c = {}
    for (w, h), seed in SHAPES.items():
        c["shape_%dx%d" % (w, h)] = ("shapes", lambda w=w, h=h, seed=seed: (records(noise(w, h, seed)), w, h))
    c["shape_step_3x3"] = ("shapes", step_3x3)
    for o in SEAM_ORIENTATIONS:
        for last in (0, 1):
            for ox in SEAM_OFFSETS:
                for oy in SEAM_OFFSETS:
                    c["seam_%s_%s_%d_%d" % (o, "last" if last else "first", ox, oy)] = ("seams", lambda o=o, last=last, ox=ox, oy=oy: seam(o, last, ox, oy))
    for o in ("vertical", "horizontal"):
        for top in ("strong", "below_strong"):
            for bottom in ("weak", "below_weak"):
                for gap in (0, 3):
                    c["two_level_%s_%s_%s_gap%d" % (o, top, bottom, gap)] = (
                        "two_level", lambda o=o, top=top, bottom=bottom, gap=gap: two_level(o, just(o)[top], just(o)[bottom], gap))
    c["exact_step"] = ("exact", exact_step)
    c["exact_step_T"] = ("exact", lambda: exact_step(True))
    for base in EXACT_BASES:
        for v in EXACT_VARIANTS:
            c["exact_fade_%d_%s" % (base, v)] = ("exact", lambda base=base, v=v: exact_fade(base, v))
    for kind in ("x", "y", "checker", "slant"):
        for k in (2, 3):
            for lo, hi in ((0, 255), (13, 200), (40, 77)):
                c["ties_%s%d_%d_%d" % (kind, k, lo, hi)] = ("ties", lambda kind=kind, k=k, lo=lo, hi=hi: bars(kind, k, lo, hi))
    for a, b in PLANE_SLOPES:
        c["plane_%d_%d" % (a, b)] = ("directions", lambda a=a, b=b: plane(a, b))
    for deg in R.CLASS_BOUNDARIES:
        c["plane_at_%g" % deg] = ("directions", lambda deg=deg: plane(7 * math.cos(math.radians(deg)), 7 * math.sin(math.radians(deg))))
        for d in (-1.0, 0.0, 1.0):
            c["step_at_%g" % (deg + d)] = ("directions", lambda deg=deg, d=d: angled_step(deg + d))
    base = lambda: records(noise(97, 70, SHAPES[(97, 70)]))
    rng = lambda: np.random.default_rng(17)
    c["records_stride20"] = ("records", lambda: (restride(base(), POINT20), 97, 70))
    c["records_stride48"] = ("records", lambda: (restride(base(), POINT48), 97, 70))
    c["records_alpha"] = ("records", lambda: (records(noise(97, 70, SHAPES[(97, 70)]), alpha=rng().integers(0, 256, 97 * 70)), 97, 70))
    c["records_non_finite"] = ("records", lambda: (scattered_non_finite(base()), 97, 70))
    c["records_non_finite_stride20"] = ("records", lambda: (restride(scattered_non_finite(base()), POINT20), 97, 70))
    for ch in ("r", "b", "alpha", "x"):
        c["records_only_" + ch] = ("records", lambda ch=ch: one_channel(ch))
    for kind in ("first", "last", "first_and_last", "dense"):
        c["compaction_" + kind] = ("compaction", lambda kind=kind: compaction(kind))
    c["compaction_flat"] = ("compaction", lambda: (records(np.full((COMPACT_H, COMPACT_W), 128)), COMPACT_W, COMPACT_H))
    return c


CASES = _cases()
GROUPS = ("shapes", "seams", "two_level", "exact", "ties", "directions", "records", "compaction")


def names(*groups):
    return [n for n, (g, _) in CASES.items() if g in groups]


def build(name):
    pts, w, h = CASES[name][1]()
    assert len(pts) == w * h
    return pts, w, h


@functools.lru_cache(maxsize=None)
def indices(name):
    pts, w, h = build(name)
    idx = R.edge_indices(pts, w, h)
    idx.flags.writeable = False
    return idx


def stages(name):
    pts, w, h = build(name)
    return R.canny(pts["rgba"], w, h)


@functools.lru_cache(maxsize=None)
def threshold_sweep(orientation):
    """delta -> (largest magnitude of an interior pixel, number of edge points) for the step of every height"""
    out = []
    for delta in range(256):
        pts, w, h = threshold_step(orientation, delta)
        s = R.canny(pts["rgba"], w, h)
        out.append((float(s.mag[1:-1, 1:-1].max()), len(s.indices)))
    return out


@functools.lru_cache(maxsize=None)
def just(orientation):
    """the step heights on either side of the two thresholds: the smallest whose largest interior magnitude is not below 40
    ('weak') and not below 100 ('strong'), and the heights one below them"""
    mags = [m for m, _ in threshold_sweep(orientation)]
    weak = min(d for d in range(256) if not mags[d] < 40.0)
    strong = min(d for d in range(256) if not mags[d] < 100.0)
    return {"weak": weak, "below_weak": weak - 1, "strong": strong, "below_strong": strong - 1}
