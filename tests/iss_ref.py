"""A reference of pcl::ISSKeypoint3D as include/rsreg.h defines it (rsreg_cloud_iss_saliency, rsreg_cloud_iss_non_max,
rsreg_cloud_iss_keypoints), numpy and tests/radius_ref.py only, independent of the engine:

  * both neighbourhoods are radius_ref.search's: float32 d2 < float32(float64(r) * float64(r)), strictly, the record itself and
    exact copies among them, the finite records only;
  * scatter: S = sum d d^T over the neighbours within the salient radius, d = float64(neighbour) - float64(record); not divided,
    not centred; zero when the record has fewer than min_neighbors neighbours;
  * eigenvalues: numpy.linalg.eigvalsh, ascending (the engine: a cyclic Jacobi -- they agree to the rounding of the solve);
  * saliency: l3 where all three are finite, l3 >= 0, l2 / l1 < gamma_21 and l3 / l2 < gamma_32 (a NaN ratio fails), else 0;
  * non-maximum suppression: a keypoint iff saliency > 0, the count at the non-max radius >= min_neighbors, and no neighbour
    within that radius has a LARGER saliency (strict: ties stay; a NaN neither is above 0 nor exceeds anything).  Vectorised over the
    flat neighbour list: the largest saliency among a record's neighbours, NaN taken as -inf, decides.

Exact copies ask the same question and get the same answer (radius_ref: one query per distinct point)."""
import numpy as np

import radius_ref as R

PRODUCTS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def scatter(xyz, nb, min_neighbors=0):
    """(S (n, 3, 3) float64, m (n,) uint32): every record's scatter over the neighbours `nb` holds; zeros where m < min_neighbors
    and for a non-finite record."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    p = xyz.astype(np.float64)
    nq = len(nb.q)
    Sq = np.zeros((nq, 3, 3))
    if nq:
        lens = np.diff(nb.off)
        rows = np.repeat(np.arange(nq), lens)
        d = p[nb.idx] - nb.q.astype(np.float64)[rows]
        first = nb.off[:-1]                                   # (every distinct point has itself: no empty row)
        for a, b in PRODUCTS:                                 # one product at a time: the flat list of a frame has 10^7 entries
            Sq[:, a, b] = Sq[:, b, a] = np.add.reduceat(d[:, a] * d[:, b], first)
        Sq[lens < min_neighbors] = 0.0
    S = np.zeros((len(xyz), 3, 3))
    S[nb.fin] = Sq[nb.inv]
    return S, nb.counts()


def saliency_rule(eig, gamma_21, gamma_32):
    """The threshold rule on ascending eigenvalues (n, 3): IEEE float64 divisions, a NaN ratio fails its compare."""
    eig = np.asarray(eig, np.float64)
    l3, l2, l1 = eig[:, 0], eig[:, 1], eig[:, 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = np.isfinite(eig).all(axis=1) & (l3 >= 0) & (l2 / l1 < gamma_21) & (l3 / l2 < gamma_32)
    return np.where(ok, l3, 0.0)


def non_max(saliency, nb, min_neighbors):
    """bool per record: the keypoints among the given saliencies, `nb` the neighbours within the non-max radius."""
    sal = np.asarray(saliency, np.float64)
    out = np.zeros(len(sal), bool)
    if not len(nb.q):
        return out
    cmp = np.where(np.isnan(sal), -np.inf, sal)               # a NaN neighbour exceeds nothing
    top = np.maximum.reduceat(cmp[nb.idx], nb.off[:-1])       # per distinct point: the largest saliency within the radius
    fin = np.flatnonzero(nb.fin)
    with np.errstate(invalid="ignore"):
        mine = sal[fin]
        out[fin] = (mine > 0) & (nb.counts()[fin] >= min_neighbors) & ~(mine < top[nb.inv])
    return out


class Iss:
    """S, eig (ascending), trace, m_s, m_n, saliency, keypoint (bool), indices; nb_s, nb_n: the two searches."""


def detect(xyz, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, nb_s=None, nb_n=None):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    r = Iss()
    r.nb_s = nb_s if nb_s is not None else R.search(xyz, salient_radius)
    r.nb_n = nb_n if nb_n is not None else R.search(xyz, non_max_radius)
    r.S, r.m_s = scatter(xyz, r.nb_s, min_neighbors)
    r.trace = np.trace(r.S, axis1=1, axis2=2)
    r.eig = np.linalg.eigvalsh(r.S)
    r.saliency = saliency_rule(r.eig, gamma_21, gamma_32)
    r.m_n = r.nb_n.counts()
    r.keypoint = non_max(r.saliency, r.nb_n, min_neighbors)
    r.indices = np.flatnonzero(r.keypoint).astype(np.int32)
    r.gammas, r.min_neighbors = (gamma_21, gamma_32), min_neighbors
    return r


def fragile(r):
    """bool per record: membership may differ between two correct implementations whose eigenvalues differ by B = 1e-12 * trace
    (the bound of the eigenvalue check).  A record is fragile when
      (a) a ratio lies within 4 B / denominator of its gamma (numerator and denominator move by B each, the ratio is below 1:
          2 B / denominator, doubled),
      (b) l3 <= B (the tests l3 >= 0 and saliency > 0),
      (c) a neighbour within the non-max radius is fragile by (a) or (b) (its saliency may be 0 on one side and l3 on the other),
      (d) its saliency is within B_i + B_j of that of a neighbour j at another place (an exact copy has the same saliency on both
          sides) -- a pair of two zeros decides nothing and is not counted.
    Records with a zero scatter (below min_neighbors, not finite, every neighbour in one place) are exact on both sides."""
    eig, B = r.eig, 1e-12 * r.trace
    l3, l2, l1 = eig[:, 0], eig[:, 1], eig[:, 2]
    live = r.trace > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        a = live & ((np.abs(l2 / l1 - r.gammas[0]) <= 4 * B / l1) | (np.abs(l3 / l2 - r.gammas[1]) <= 4 * B / l2))
    b = live & (l3 <= B)
    own = a | b
    nb = r.nb_n
    out = own.copy()
    if len(nb.q):
        fin = np.flatnonzero(nb.fin)
        first = nb.off[:-1]
        c = np.logical_or.reduceat(own[nb.idx], first)
        rep = np.zeros(len(nb.q), np.int64)                   # a record of every distinct point (they share saliency and B)
        rep[nb.inv] = fin
        rows = np.repeat(np.arange(len(nb.q)), np.diff(nb.off))
        si, sj = r.saliency[rep][rows], r.saliency[nb.idx]
        fin_of = np.full(len(r.saliency), -1, np.int64)
        fin_of[fin] = nb.inv
        elsewhere = fin_of[nb.idx] != rows
        close = elsewhere & ((si != 0) | (sj != 0)) & (np.abs(si - sj) <= B[rep][rows] + B[nb.idx])
        d = np.logical_or.reduceat(close, first)
        out[fin] |= (c | d)[nb.inv]
    return out
