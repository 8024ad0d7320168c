"""The reference of the ICP correspondence search (rsreg_icp_search, rsreg_icp_sums), on the CPU: the brute force of
tests/test_nn_fuzz_gpu.py::brute in chunks, and the 17 sums of the accepted pairs in exact arithmetic.

  d2        float32, FLANN's L2_Simple order (dx * dx + dy * dy) + dz * dz, every operation rounded once (IEEE: a difference that
            overflows gives +inf, a square that underflows a denormal or 0);
  nearest   the lowest target index among the smallest d2 (+inf ties with +inf); non-finite target records do not take part;
  gate      a pair is rejected iff (double)d2 > gate * gate (PCL: if (distance > max_dist_sqr) continue);
  -1        for a non-finite source record, for a rejected pair, and where no target record is finite.

UNBOUNDED is PCL's default gate, sqrt(DBL_MAX): its square is a finite double, so a pair at d2 = +inf is rejected.

The 17 sums (include/rsreg.h, RSREG_NUM_SUMS), p the source record and q its match, as doubles of the float32 values, every source
record counting once (exact copies of a point are records like any other: the weight of a pair is the number of records it
stands for):  [0] n   [1..3] sum p   [4..6] sum q   [7..15] sum q_i * p_j   [16] sum (double)d2.
A product of two float32 values is an exact double, so every term is one, and math.fsum returns the correctly rounded sum;
`sums_abs` holds sum |term| per entry, the scale of the header's bound on a sum of N terms, (N + 16) 2^-53 sum |term|.
"""
import collections
import math

import numpy as np

UNBOUNDED = math.sqrt(np.finfo(np.float64).max)

Result = collections.namedtuple("Result", "idx d2 near_idx near_d2 sums sums_abs")


def finite_rows(xyz):
    return np.isfinite(np.asarray(xyz, np.float32)).all(axis=1)


def d2_f32(a, b):
    """L2_Simple of broadcastable float32 arrays (..., 3)."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        d = (a - b).astype(np.float32)
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        return (((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32) + (dz * dz).astype(np.float32)).astype(np.float32)


def nearest(src, tgt, chunk=128):
    """(index into tgt or -1, float32 d2) of every source record's nearest finite target record, whatever the gate."""
    s, t = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    idx = np.full(len(s), -1, np.int64)
    d2o = np.zeros(len(s), np.float32)
    ti = np.flatnonzero(finite_rows(t))
    tt = t[ti]
    if len(tt) == 0:
        return idx, d2o
    ok = np.flatnonzero(finite_rows(s))
    for a in range(0, len(ok), chunk):
        rows = ok[a:a + chunk]
        d2 = d2_f32(s[rows][:, None, :], tt[None, :, :])
        assert not np.isnan(d2).any()
        j = np.argmin(d2, axis=1)                  # the first minimum: the lowest index
        idx[rows] = ti[j]
        d2o[rows] = d2[np.arange(len(rows)), j]
    return idx, d2o


def sums_of(src, tgt, idx, d2):
    """The 17 sums of the pairs idx >= 0, correctly rounded, and sum |term| per entry."""
    s, t = np.asarray(src, np.float32).reshape(-1, 3).astype(np.float64), np.asarray(tgt, np.float32).reshape(-1, 3).astype(np.float64)
    rows = np.flatnonzero(idx >= 0)
    P, Q = s[rows], t[idx[rows]]
    cols = [np.ones(len(rows))] + [P[:, k] for k in range(3)] + [Q[:, k] for k in range(3)]
    cols += [Q[:, r] * P[:, c] for r in range(3) for c in range(3)]          # exact: 24 x 24 bits
    cols += [np.asarray(d2, np.float32)[rows].astype(np.float64)]
    sums = np.array([math.fsum(c.tolist()) for c in cols])
    sums_abs = np.array([math.fsum(np.abs(c).tolist()) for c in cols])
    return sums, sums_abs


def search(src, tgt, gate):
    near_idx, near_d2 = nearest(src, tgt)
    gate2 = float(gate) * float(gate)
    keep = (near_idx >= 0) & ~(near_d2.astype(np.float64) > gate2)
    idx = np.where(keep, near_idx, -1)
    d2 = np.where(keep, near_d2, np.float32(0)).astype(np.float32)
    sums, sums_abs = sums_of(src, tgt, idx, d2)
    for a in (idx, d2, near_idx, near_d2, sums, sums_abs):
        a.setflags(write=False)
    return Result(idx, d2, near_idx, near_d2, sums, sums_abs)


def sums_bound(ref):
    """Per entry: (N + 16) 2^-53 sum |term|, N the number of accepted pairs (include/rsreg.h)."""
    n = int((ref.idx >= 0).sum())
    return (n + 16) * 2.0 ** -53 * ref.sums_abs
