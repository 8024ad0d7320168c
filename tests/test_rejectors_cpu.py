"""The rejector chain's numpy reference (tests/rejectors_ref.py) against an independent restatement in plain Python loops, and
the chain's structs and constants in the ctypes mirror against include/rsreg.h.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rejectors_ref as J
from test_filters import _np_filters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _loops(idx, d2, chain, sn, tn):
    """apply_chain record by record: no sorts of index arrays, no vector arithmetic."""
    idx = [int(v) for v in idx]
    n = len(idx)
    stats = []
    for kind, value in chain:
        play = [i for i in range(n) if idx[i] >= 0]
        m, med = len(play), 0.0
        if kind == J.MEDIAN_DISTANCE:
            if m:
                med = sorted(float(d2[i]) for i in play)[m // 2]          # (a float32 is a float64: the order is the same)
                for i in play:
                    if not float(d2[i]) <= med * float(value):
                        idx[i] = -1
        elif kind == J.ONE_TO_ONE:
            best = {}
            for i in play:                                                # ascending index: a strict `<` leaves ties to the lowest
                t = idx[i]
                if t not in best or d2[i] < d2[best[t]]:
                    best[t] = i
            for i in play:
                if best[idx[i]] != i:
                    idx[i] = -1
        elif kind == J.SURFACE_NORMAL:
            for i in play:
                s, t = sn[i], tn[idx[i]]
                with np.errstate(invalid="ignore", over="ignore"):
                    score = f32(f32(f32(s[0]) * f32(t[0])) + f32(f32(s[1]) * f32(t[1]))) + f32(f32(s[2]) * f32(t[2]))
                if not float(score) > float(value):
                    idx[i] = -1
        elif kind == J.TRIMMED:
            keep = int(np.floor(f32(value) * f32(m)))
            if keep < m:
                for i in sorted(play, key=lambda i: (float(d2[i]), i))[keep:]:
                    idx[i] = -1
        stats.append((m, sum(1 for v in idx if v >= 0), float(med)))
    return np.array(idx, np.int32), stats


def _pairs(seed):
    """900 source records over 700 target records with ten copied records, their pairs within the gate, unit normals on both sides
    (the copies carry different ones) and a few NaN normals."""
    rng = np.random.default_rng(seed)
    tgt = rng.random((700, 3)).astype(np.float32)
    src = (tgt[rng.integers(0, 700, 900)] + rng.normal(0, 0.02, (900, 3))).astype(np.float32)
    src[100:110] = src[100]
    idx, d2 = _np_filters(src, tgt, 0.05, 0, 0.0)
    tn = rng.normal(size=(700, 3))
    tn = (tn / np.linalg.norm(tn, axis=1)[:, None]).astype(np.float32)
    sn = (tn[np.maximum(idx, 0)] + rng.normal(0, 0.5, (900, 3))).astype(np.float32)
    sn = (sn / np.linalg.norm(sn, axis=1)[:, None]).astype(np.float32)
    sn[rng.choice(900, 5, replace=False), 1] = np.nan
    tn[rng.choice(700, 5, replace=False), 2] = np.nan
    return idx, d2, sn, tn


CHAINS = {
    "median": [(1, 1.0)], "median-1.5": [(1, 1.5)], "one-to-one": [(2, 0.0)], "normal": [(3, 0.8)], "trimmed": [(4, 0.6)],
    "median,one-to-one": [(1, 1.0), (2, 0.0)], "one-to-one,median": [(2, 0.0), (1, 1.0)],
    "normal,median": [(3, 0.5), (1, 1.0)], "trimmed,one-to-one": [(4, 0.7), (2, 0.0)],
}


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("seed", [5, 6])
def test_reference_matches_loops(name, seed):
    idx, d2, sn, tn = _pairs(seed)
    assert (idx >= 0).sum() > 500 and len(set(idx[100:110])) == 1 and idx[100] >= 0      # the copies are in play, on one target
    got, gs = J.apply_chain(idx, d2, CHAINS[name], sn, tn)
    want, ws = _loops(idx, d2, CHAINS[name], sn, tn)
    np.testing.assert_array_equal(got, want)
    assert gs == ws
    assert 0 < (got >= 0).sum() < (idx >= 0).sum()                                         # every chain here removes pairs, none all


@pytest.mark.parametrize("seed", [5, 6])
def test_order_matters(seed):
    idx, d2, sn, tn = _pairs(seed)
    a, _ = J.apply_chain(idx, d2, CHAINS["median,one-to-one"], sn, tn)
    b, _ = J.apply_chain(idx, d2, CHAINS["one-to-one,median"], sn, tn)
    assert (a != b).any()


def test_copies_with_different_normals_split():
    """Ten records at one point, one target: the normal test keeps the copies whose own normal passes, wherever they stand."""
    idx = np.full(10, 3, np.int32)
    d2 = np.full(10, 0.25, np.float32)
    tn = np.zeros((4, 3), np.float32)
    tn[3] = (0, 0, 1)
    sn = np.zeros((10, 3), np.float32)
    sn[:, 2] = [1, 0, 1, 0.5, 1, np.nan, 0.75, 0.5, 1, 0]
    got, st = J.apply_chain(idx, d2, [(3, 0.5)], sn, tn)
    np.testing.assert_array_equal(got >= 0, [1, 0, 1, 0, 1, 0, 1, 0, 1, 0])          # 0.5 > 0.5 is false: the comparison is strict
    assert st == [(10, 5, 0.0)]
    got, st = J.apply_chain(idx, d2, [(3, 0.5), (2, 0.0)], sn, tn)
    np.testing.assert_array_equal(np.nonzero(got >= 0)[0], [0])


def test_median_edges():
    d2 = np.array([0, 1, 1, 1, 4, np.inf], np.float32)
    idx = np.arange(6, dtype=np.int32)
    got, st = J.apply_chain(idx, d2, [(1, 1.0)])
    assert st == [(6, 4, 1.0)] and (got >= 0).tolist() == [True] * 4 + [False] * 2        # rank 3 of 6: the upper median, the bound kept
    got, st = J.apply_chain(idx, d2, [(1, 0.0)])
    assert st == [(6, 1, 1.0)] and got[0] == 0
    got, st = J.apply_chain(idx[5:], d2[5:], [(1, 0.0)])                                   # inf * 0: NaN drops everything
    assert st == [(1, 0, float("inf"))]
    got, st = J.apply_chain(np.full(3, -1, np.int32), d2[:3], [(1, 1.0), (2, 0.0)])
    assert st == [(0, 0, 0.0), (0, 0, 0.0)]
    got, st = J.apply_chain(idx[:2], d2[:2], [(1, 1.0)])                                   # m = 2: rank 1, both stay
    assert st == [(2, 2, 1.0)]


def test_rotate_normals_restates_float32():
    rng = np.random.default_rng(3)
    n = rng.normal(size=(50, 3)).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = rng.normal(size=(3, 3)).astype(np.float32)
    T[:3, 3] = (5, 6, 7)                                                                   # the translation is not applied
    got = J.rotate_normals(n, T)
    for i in range(50):
        for r in range(3):
            assert got[i, r] == f32(f32(f32(T[r, 0] * n[i, 0]) + f32(T[r, 1] * n[i, 1])) + f32(T[r, 2] * n[i, 2]))


# ---- the ABI's new structs and constants
@pytest.fixture(scope="module")
def L(rs):
    from rsreg_amd import lib
    return lib


def test_rejector_structs_match_header(L):
    hdr = open(os.path.join(ROOT, "include", "rsreg.h")).read()
    assert "typedef struct rsreg_rejector { int32_t kind; int32_t reserved0; double value; } rsreg_rejector;" in hdr
    assert "typedef struct rsreg_rejector_stat { uint64_t n_in, n_out; double median_distance; double reserved0; } rsreg_rejector_stat;" in hdr
    assert C.sizeof(L.Rejector) == 16 and C.sizeof(L.RejectorStat) == 32
    assert [(n, getattr(L.Rejector, n).offset) for n, _ in L.Rejector._fields_] == [("kind", 0), ("reserved0", 4), ("value", 8)]
    assert [(n, getattr(L.RejectorStat, n).offset) for n, _ in L.RejectorStat._fields_] == [("n_in", 0), ("n_out", 8), ("median_distance", 16), ("reserved0", 24)]
    kinds = dict(re.findall(r"RSREG_REJECTOR_([A-Z_]+?)\s*=\s*(\d+)", hdr))
    assert {k: int(v) for k, v in kinds.items()} == {"MEDIAN_DISTANCE": L.REJECTOR_MEDIAN_DISTANCE, "ONE_TO_ONE": L.REJECTOR_ONE_TO_ONE,
                                                      "SURFACE_NORMAL": L.REJECTOR_SURFACE_NORMAL, "TRIMMED": L.REJECTOR_TRIMMED}
    assert (J.MEDIAN_DISTANCE, J.ONE_TO_ONE, J.SURFACE_NORMAL, J.TRIMMED) == (1, 2, 3, 4)
    assert int(re.search(r"#define RSREG_MAX_REJECTORS (\d+)", hdr).group(1)) == L.MAX_REJECTORS == 8
    for name in ("rsreg_icp_set_rejectors", "rsreg_icp_rejector_stats", "rsreg_icp_set_source_normals", "rsreg_icp_set_source_normals_cloud"):
        assert name in L.EXPORTS


def test_python_surface(rs):
    """The PCL-named classes carry kind and value; the chain keeps its order and its limit."""
    from rsreg_amd import api, lib
    m, o, s, t = (api.CorrespondenceRejectorMedianDistance(), api.CorrespondenceRejectorOneToOne(), api.CorrespondenceRejectorSurfaceNormal(),
                  api.CorrespondenceRejectorTrimmed())
    assert (m.getMedianFactor(), s.getThreshold(), m.getMedianDistance()) == (1.0, 1.0, 0.0)       # PCL's defaults
    m.setMedianFactor(2.5), s.setThreshold(0.25), t.setOverlapRatio(0.75)
    assert [(r.kind, r.value) for r in (m, o, s, t)] == [(1, 2.5), (2, 0.0), (3, 0.25), (4, 0.75)] and t.getOverlapRatio() == 0.75
    icp = api.IterativeClosestPoint.__new__(api.IterativeClosestPoint)                              # (no context: no GPU here)
    icp._rejectors = []
    for r in (o, m):
        icp.addCorrespondenceRejector(r)
    assert icp.getCorrespondenceRejectors() == [o, m]
    assert icp.removeCorrespondenceRejector(0) and icp.getCorrespondenceRejectors() == [m] and not icp.removeCorrespondenceRejector(5)
    for _ in range(7):
        icp.addCorrespondenceRejector(api.CorrespondenceRejectorOneToOne())
    with pytest.raises(lib.RsregError):
        icp.addCorrespondenceRejector(o)
    icp.clearCorrespondenceRejectors()
    assert icp.getCorrespondenceRejectors() == []
    with pytest.raises(ValueError):
        icp.addCorrespondenceRejector(api.CorrespondenceRejector())
