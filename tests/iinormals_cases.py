"""Inputs of tests/test_iinormals_cpu.py and tests/test_iinormals_gpu.py: organized frames as (h, w, 3) float32 arrays."""
import numpy as np

Q = 2.0 ** -12


def quantised_cloud(w=96, h=64, seed=11):
    """Coordinates that are multiples of 2^-12 below 16: every window sum is exact in double, whatever its order.  A depth step at
    column 60, a block of records at the origin, 60 NaN records and one Inf."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x = (c - w // 2) * 2.0 ** -6 + rng.integers(-8, 9, (h, w)) * Q
    y = (r - h // 2) * 2.0 ** -6 + rng.integers(-8, 9, (h, w)) * Q
    z = 1.5 + np.round((0.2 * np.sin(c / 9.0) + 0.1 * np.cos(r / 7.0)) / Q) * Q + rng.integers(-4, 5, (h, w)) * Q
    z[:, 60:] += 0.5
    P = np.stack([x, y, z], axis=2)
    P[20:29, 10:21] = 0.0
    holes = rng.choice(w * h, 60, replace=False)
    P.reshape(-1, 3)[holes] = np.nan
    P[40, 70, 2] = np.inf
    assert (np.abs(P[np.isfinite(P)]) < 16).all()
    P = P.astype(np.float32)
    fin = np.isfinite(P)
    assert (P[fin] / Q == np.round(P[fin] / Q)).all()
    return P


def spike_frame(w, h, rows):
    """Flat depth 1 with single spikes of depth 2: the four corners, the middle of each border column and row, two columns of
    each row of `rows` (the rows on both sides of the passes' band boundaries)."""
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    P = np.stack([(c - w / 2) * 0.01, (r - h / 2) * 0.01, np.ones((h, w))], axis=2).astype(np.float32)
    at = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, 0), (h // 2, w - 1), (0, w // 2), (h - 1, w // 3)]
    for k, row in enumerate(rows):
        if 0 <= row < h:
            at += [(row, (7 + 13 * k) % w), (row, (w - 5 - 11 * k) % w)]
    for rr, cc in at:
        P[rr, cc, 2] = 2.0
    return P


def plane_frame(w, h, a, b, c, step=2.0 ** -7):
    """z = a x + b y + c on a pixel grid of spacing `step` (a, b, c and step powers of two or sums of a few: exact in float32)."""
    r, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x, y = (cc - w // 2) * step, (r - h // 2) * step
    return np.stack([x, y, a * x + b * y + c], axis=2).astype(np.float32)
