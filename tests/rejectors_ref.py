"""A numpy reference of the ICP rejector chain (include/rsreg.h: rsreg_icp_set_rejectors), independent of the engine: the pairs
in play come in as (target index or -1, float32 d2) per source record in the caller's order -- what a search without a chain
returns -- and every rejector runs over what the one before left.

  MEDIAN_DISTANCE  median = the d2 at rank floor(m / 2) of the m pairs in play, ascending; kept iff double(d2) <= double(median) * factor
  ONE_TO_ONE       of the pairs that share a target record the smallest (d2, source index) stays
  SURFACE_NORMAL   kept iff double((sx*tx + sy*ty) + sz*tz) > threshold, the dot product in float32, each operation rounded once
  TRIMMED          filters_ref.trim_keep(ratio, m) pairs stay, in (d2, source index) order
"""
import numpy as np

import filters_ref as R

MEDIAN_DISTANCE, ONE_TO_ONE, SURFACE_NORMAL, TRIMMED = 1, 2, 3, 4


def rotate_normals(n, T):
    """The normals under the 3 x 3 block of T in float32: x' = (r0*x + r1*y) + r2*z, no fused operations, no translation."""
    n = np.asarray(n, np.float32)
    T = np.asarray(T, np.float32)
    out = np.empty_like(n)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            out[:, r] = (T[r, 0] * n[:, 0] + T[r, 1] * n[:, 1]) + T[r, 2] * n[:, 2]
    return out


def normal_scores(s, t):
    """getCorrespondenceScoreFromNormals in float32 for rows of source and target normals."""
    s, t = np.asarray(s, np.float32), np.asarray(t, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (s[:, 0] * t[:, 0] + s[:, 1] * t[:, 1]) + s[:, 2] * t[:, 2]


def apply_chain(idx, d2, chain, src_normals_cur=None, tgt_normals=None):
    """(kept index per source record, -1 where the chain dropped the pair; [(n_in, n_out, median d2)] per entry).
    chain: [(kind, value)]; src_normals_cur: the source records' normals as they stand now, (n, 3) float32; tgt_normals: one
    per target record."""
    idx = np.asarray(idx).astype(np.int64).copy()
    d2 = np.asarray(d2, np.float32)
    stats = []
    for kind, value in chain:
        play = np.nonzero(idx >= 0)[0]
        m = len(play)
        med = 0.0
        if kind == MEDIAN_DISTANCE:
            if m:
                med = np.sort(d2[play])[m // 2]
                with np.errstate(invalid="ignore", over="ignore"):
                    bound = np.float64(med) * np.float64(value)
                    keep = d2[play].astype(np.float64) <= bound
                idx[play[~keep]] = -1
        elif kind == ONE_TO_ONE:
            order = play[np.lexsort((play, d2[play], idx[play]))]
            t = idx[order]
            lead = np.r_[True, t[1:] != t[:-1]] if m else np.zeros(0, bool)
            idx[order[~lead]] = -1
        elif kind == SURFACE_NORMAL:
            score = normal_scores(src_normals_cur[play], tgt_normals[idx[play]])
            with np.errstate(invalid="ignore"):
                keep = score.astype(np.float64) > float(value)
            idx[play[~keep]] = -1
        elif kind == TRIMMED:
            keep_n = R.trim_keep(value, m)
            if keep_n < m:
                order = play[np.lexsort((play, d2[play]))]
                idx[order[keep_n:]] = -1
        else:
            raise ValueError(kind)
        stats.append((m, int((idx >= 0).sum()), float(med)))
    return idx.astype(np.int32), stats
