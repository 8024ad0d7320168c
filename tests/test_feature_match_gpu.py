"""rsreg_cloud_feature_knn and rsreg_cloud_feature_correspondences (the exact k-NN in FPFH space and
pcl::registration::CorrespondenceEstimation over it) on the GPU, the Python and C++ adaptors, against tests/feature_match_ref.py.

Indices, squared distances and correspondence lists are BIT-EQUAL to the reference on every row of every case: the contract
(include/rsreg.h) fixes the operation order and the tie rule, so there is no tolerance and no set of rows that is let off.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import feature_match_cases as K
import feature_match_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    return api


@pytest.fixture(scope="module")
def ctx(api):
    return api.Context(0)


def _dev(api, ctx, rows, stride=132, seed=0):
    """The rows as a device cloud of `stride`-byte records, random bits behind the 33 floats"""
    return api.DeviceCloud(api.FPFHCloud(K.records(rows, stride, seed), len(rows), 1, True), ctx=ctx)


def _host(api, rows):
    rec = np.zeros(len(rows), api.FPFH_DTYPE)
    rec["histogram"] = rows
    return api.FPFHCloud(rec, len(rec), 1, True)


POOLS = {"exact": K.exact, "order": K.order, "real": K.real}


@functools.lru_cache(maxsize=None)
def _pool_d2(name):
    src, tgt = POOLS[name]()
    return R.d2_matrix(src, tgt)


_CLOUDS = {}


def _prefix(api, ctx, name, role, n):
    """The first n rows of a pool's source (role 0) or target (role 1) in HBM, uploaded once"""
    key = (name, role, n)
    if key not in _CLOUDS:
        _CLOUDS[key] = _dev(api, ctx, POOLS[name]()[role][:n])
    return _CLOUDS[key]


def _check_knn(api, ctx, src, tgt, k, d2=None, dsrc=None, dtgt=None, label=""):
    d2 = R.d2_matrix(src, tgt) if d2 is None else d2
    want_i, want_d = R.knn_from_d2(d2, R.valid_rows(src), R.valid_rows(tgt), k)
    dsrc = dsrc or _dev(api, ctx, src)
    dtgt = dtgt or _dev(api, ctx, tgt)
    idx, dist = dsrc.feature_knn(dtgt, k)
    assert idx.shape == (len(src), k) and idx.dtype == np.int32 and dist.shape == (len(src), k) and dist.dtype == np.float32
    bad = np.flatnonzero((idx != want_i).any(axis=1) | (dist.view(np.uint32) != want_d.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (label, len(src), len(tgt), k, bad[:4], idx[bad[:2]], want_i[bad[:2]], dist[bad[:2]], want_d[bad[:2]])
    return idx, dist


@pytest.mark.parametrize("k", K.KS + K.KS_EDGE)
@pytest.mark.parametrize("name", ["exact", "order"])
def test_knn_bit_equal_on_the_size_grid(api, ctx, name, k):
    """ns in {1, 63, 64, 65, 1000} x nt in {k, tile - 1, tile, tile + 1, 2500}: prefixes of one pool, one reference matrix.  One
    slice and several (plan(1000, 2500) cuts 39, plan(1, 2500) too; every nt <= 127 is one slice)."""
    src, tgt = POOLS[name]()
    d2 = _pool_d2(name)
    slices = set()
    for ns in K.NS:
        for nt in K.nts(k):
            slices.add(K.plan(ns, nt)[1])
            _check_knn(api, ctx, src[:ns], tgt[:nt], k, d2[:ns, :nt], _prefix(api, ctx, name, 0, ns), _prefix(api, ctx, name, 1, nt), name)
    assert 1 in slices and max(slices) > 1


@pytest.mark.parametrize("k", K.KS)
def test_knn_bit_equal_on_real_rows(api, ctx, k):
    src, tgt = K.real()
    _check_knn(api, ctx, src, tgt, k, _pool_d2("real"), _prefix(api, ctx, "real", 0, len(src)), _prefix(api, ctx, "real", 1, len(tgt)), "real")


@pytest.mark.parametrize("name", ["exact", "order"])
def test_knn_every_k(api, ctx, name):
    """k = 1 .. 16, so every list length K in {1, 2, 4, 8, 16} runs with k at its first and at its last slot (k = K: the k-th answer
    is the slot the guard and the eviction work on, no slack behind it).  (65, 2500): 39 slices and a second query block with one
    live lane; (1000, 65): one slice, a full tile and a tile of one row."""
    src, tgt = POOLS[name]()
    d2 = _pool_d2(name)
    for ns, nt in K.EVERY_K_SIZES:
        assert (K.plan(ns, nt)[1] > 1) == (nt == 2500)
        for k in range(1, 17):
            _check_knn(api, ctx, src[:ns], tgt[:nt], k, d2[:ns, :nt], _prefix(api, ctx, name, 0, ns), _prefix(api, ctx, name, 1, nt), name)


@pytest.mark.parametrize("ns,nt", K.COPIES_SIZES)
def test_knn_copies_lowest_index_wins(api, ctx, ns, nt):
    """Equal rows at index 0, tile - 1, tile and at both ends of every slice: (1, 20 000) is one query block and 312 slices,
    (3000, 16) 47 blocks and one partial tile."""
    src, tgt, planted = K.copies(ns, nt, 200 + ns)
    dsrc, dtgt = _dev(api, ctx, src), _dev(api, ctx, tgt)
    d2 = R.d2_matrix(src, tgt)
    for k in K.KS + K.KS_EDGE:
        if k > nt:
            continue
        idx, dist = _check_knn(api, ctx, src, tgt, k, d2, dsrc, dtgt, "copies")
        if k <= len(planted):
            assert idx[0].tolist() == planted[:k].tolist() and (dist[0] == 0).all()
            assert idx[ns // 2].tolist() == planted[:k].tolist()


@pytest.mark.parametrize("k", K.KS + K.KS_EDGE)
def test_knn_holes(api, ctx, k):
    """NaN, +inf, -inf in the first or last bin: never a match, never a query; a target with exactly k valid rows is searched, one
    with k - 1 refused."""
    src, tgt = K.holes()
    idx, dist = _check_knn(api, ctx, src, tgt, k, label="holes")
    bad = ~R.valid_rows(src)
    assert (idx[bad] == -1).all() and (dist[bad] == 0).all() and not np.isin(idx, np.flatnonzero(~R.valid_rows(tgt))).any()
    dsrc = _dev(api, ctx, src)
    _check_knn(api, ctx, src, K.few_valid(k), k, dsrc=dsrc, label="exactly k valid")
    from rsreg_amd import lib
    with pytest.raises(lib.RsregError) as e:
        dsrc.feature_knn(_dev(api, ctx, K.few_valid(k - 1)), k)
    assert e.value.status == lib.RSREG_ERR_INVALID_ARG


def test_strides(api, ctx):
    """132-, 144- and 160-byte records with random bits behind the row, source and target strides differing: the bytes of the
    132-byte case."""
    src, tgt = K.holes()
    first = None
    for s_stride, t_stride in ((132, 132), (144, 160), (160, 132), (132, 144)):
        dsrc, dtgt = _dev(api, ctx, src, s_stride, 1), _dev(api, ctx, tgt, t_stride, 2)
        assert dsrc.info()[1] == s_stride and dtgt.info()[1] == t_stride
        idx, dist = dsrc.feature_knn(dtgt, 5)
        got = (idx.tobytes(), dist.tobytes(), dsrc.feature_correspondences(dtgt).tobytes(), dsrc.feature_correspondences(dtgt, reciprocal=True).tobytes())
        first = first or got
        assert got == first
    want_i, want_d = R.knn(src, tgt, 5)
    assert first[0] == want_i.tobytes() and first[1] == want_d.tobytes()


def _check_lists(dsrc, dtgt, d2, sv, tv, max_distance=None, label=""):
    out = []
    for reciprocal in (False, True):
        want = R.as_records(R.correspondences_from_d2(d2, sv, tv, R.DBL_MAX if max_distance is None else max_distance, reciprocal))
        got = dsrc.feature_correspondences(dtgt, max_distance, reciprocal)
        assert got.dtype.itemsize == 12 and got.tobytes() == want.tobytes(), (label, reciprocal, len(got), len(want))
        out.append(got)
    return out


@pytest.mark.parametrize("name", ["exact", "order", "real", "holes"])
def test_correspondences_equal_the_reference(api, ctx, name):
    """Forward and reciprocal lists as bytes, at the default DBL_MAX and at a bound in the middle of the distances."""
    if name == "holes":
        src, tgt = K.holes()
        d2, dsrc, dtgt = R.d2_matrix(src, tgt), _dev(api, ctx, src), _dev(api, ctx, tgt)
    else:
        src, tgt = POOLS[name]()
        d2, dsrc, dtgt = _pool_d2(name), _prefix(api, ctx, name, 0, len(src)), _prefix(api, ctx, name, 1, len(tgt))
    sv, tv = R.valid_rows(src), R.valid_rows(tgt)
    fwd, rec = _check_lists(dsrc, dtgt, d2, sv, tv, None, name)
    assert len(fwd) == sv.sum() and 0 < len(rec) < len(fwd)
    assert (np.diff(fwd["index_query"]) > 0).all() and (np.diff(rec["index_query"]) > 0).all()
    middle = float(np.sqrt(np.float64(np.median(fwd["distance"]))))
    part, _ = _check_lists(dsrc, dtgt, d2, sv, tv, middle, name)
    assert 0 < len(part) < len(fwd)


def test_max_distance_at_the_bound(api, ctx):
    """max_distance whose square in double IS one row's d2: the row is kept.  The next float below: it is dropped.  max_distance = 0
    keeps exactly the d2 = 0 matches."""
    src, tgt = K.exact()
    d2, dsrc, dtgt = _pool_d2("exact"), _prefix(api, ctx, "exact", 0, len(src)), _prefix(api, ctx, "exact", 1, len(tgt))
    sv, tv = R.valid_rows(src), R.valid_rows(tgt)
    fwd = dsrc.feature_correspondences(dtgt)
    roots = np.sqrt(fwd["distance"].astype(np.float64))
    square = np.flatnonzero((roots * roots == fwd["distance"]) & (fwd["distance"] > 0))   # d2 whose root is a double that squares back exactly
    assert len(square) > 0
    row = fwd[square[0]]
    at = float(roots[square[0]])
    assert at * at == float(row["distance"])
    kept, _ = _check_lists(dsrc, dtgt, d2, sv, tv, at, "at the bound")
    assert row["index_query"] in kept["index_query"] and kept["distance"].max() == row["distance"]
    below = float(np.sqrt(np.float64(np.nextafter(row["distance"], np.float32(0)))))
    assert below * below < float(row["distance"])
    dropped, _ = _check_lists(dsrc, dtgt, d2, sv, tv, below, "below the bound")
    assert row["index_query"] not in dropped["index_query"] and len(dropped) < len(kept)
    # d2 = 0: the real case's source ends with 100 target rows verbatim
    rs, rt = K.real()
    zero, zero_rec = _check_lists(_prefix(api, ctx, "real", 0, len(rs)), _prefix(api, ctx, "real", 1, len(rt)), _pool_d2("real"), R.valid_rows(rs),
                                  R.valid_rows(rt), 0.0, "zero")
    assert len(zero) >= 100 and (zero["distance"] == 0).all() and (zero["index_query"][-100:] == np.arange(len(rs) - 100, len(rs))).all()
    assert (_pool_d2("real").min(axis=1) == 0).sum() == len(zero) and 0 < len(zero_rec) <= len(zero)


def test_reciprocal_tie_drops_a_good_forward_match(api, ctx):
    """Source rows at 0, 1, 10 and target rows at 0.5, 0.5, 9 along bin 0: target row 0 is as near to source row 1 as to row 0, the
    tie goes to row 0, so row 1 -- whose forward match to target 0 was good -- is not reciprocal."""
    def rows(xs):
        out = np.zeros((len(xs), 33), np.float32)
        out[:, 0] = xs
        return out
    src, tgt = rows([0.0, 1.0, 10.0]), rows([0.5, 0.5, 9.0])
    fwd, rec = _check_lists(_dev(api, ctx, src), _dev(api, ctx, tgt), R.d2_matrix(src, tgt), R.valid_rows(src), R.valid_rows(tgt), None, "tie")
    assert fwd.tolist() == [(0, 0, 0.25), (1, 0, 0.25), (2, 2, 1.0)] and rec.tolist() == [(0, 0, 0.25), (2, 2, 1.0)]


def test_overflowing_distances(api, ctx):
    """A square, a difference and a sum that overflow: d2 = +inf, which ties with every other +inf.  Source rows at +inf from every
    target row get the k lowest valid indices (against a list that starts at kFmNone); +inf matches are correspondences at DBL_MAX
    with distance inf, and exactly they are dropped at max_distance = 1e30 (its square, 1e60, is above every finite float)."""
    src, tgt = K.overflow()
    d2, dsrc, dtgt = R.d2_matrix(src, tgt), _dev(api, ctx, src), _dev(api, ctx, tgt)
    sv, tv = R.valid_rows(src), R.valid_rows(tgt)
    for k in (1, 4, 16):
        idx, dist = _check_knn(api, ctx, src, tgt, k, d2, dsrc, dtgt, "overflow")
        all_inf = np.isinf(d2).all(axis=1)
        assert all_inf.sum() >= 10 and (idx[all_inf] == np.arange(k)).all() and np.isinf(dist[all_inf]).all()
        assert not np.isnan(dist).any()
    assert (np.isfinite(dist[:, 0]) & np.isinf(dist[:, -1])).sum() >= 5
    fwd, rec = _check_lists(dsrc, dtgt, d2, sv, tv, None, "overflow")
    assert len(fwd) == len(src) and np.isinf(fwd["distance"]).sum() >= 10 and np.isinf(rec["distance"]).any()
    assert (0, 0) in zip(rec["index_query"].tolist(), rec["index_match"].tolist())     # +inf both ways, the lowest index both ways
    cut_fwd, cut_rec = _check_lists(dsrc, dtgt, d2, sv, tv, 1e30, "overflow, 1e30")
    assert cut_fwd.tobytes() == fwd[np.isfinite(fwd["distance"])].tobytes() and cut_rec.tobytes() == rec[np.isfinite(rec["distance"])].tobytes()
    assert 0 < len(cut_rec) < len(rec) and 0 < len(cut_fwd) < len(fwd)


def test_reciprocal_tie_at_infinity(api, ctx):
    """Source rows at 3e38, 2e38, 0 and target rows at -3e38, -3e38, 1 along bin 0: every d2 but the last pair's is +inf, the +inf
    ties go to index 0 both ways, so source row 1 -- whose forward match is target 0 -- is not reciprocal.  At 1e30 the +inf matches
    go, forward and reciprocal."""
    def rows(xs):
        out = np.zeros((len(xs), 33), np.float32)
        out[:, 0] = xs
        return out
    src, tgt = rows([3e38, 2e38, 0.0]), rows([-3e38, -3e38, 1.0])
    dsrc, dtgt = _dev(api, ctx, src), _dev(api, ctx, tgt)
    d2, sv, tv = R.d2_matrix(src, tgt), R.valid_rows(src), R.valid_rows(tgt)
    fwd, rec = _check_lists(dsrc, dtgt, d2, sv, tv, None, "tie at +inf")
    inf = float("inf")
    assert fwd.tolist() == [(0, 0, inf), (1, 0, inf), (2, 2, 1.0)] and rec.tolist() == [(0, 0, inf), (2, 2, 1.0)]
    fwd, rec = _check_lists(dsrc, dtgt, d2, sv, tv, 1e30, "tie at +inf, 1e30")
    assert fwd.tolist() == [(2, 2, 1.0)] and rec.tolist() == [(2, 2, 1.0)]
    idx, dist = _check_knn(api, ctx, src, tgt, 3, d2, dsrc, dtgt, "tie at +inf")
    assert idx.tolist() == [[0, 1, 2], [0, 1, 2], [2, 0, 1]]


@pytest.mark.parametrize("name", K.DENORMALS)
def test_denormal_distances(api, ctx, name):
    """d2 below FLT_MIN from normal inputs: the key is the float's bit pattern, so one flushed difference, product or sum changes
    an answer.  `zeros`: rows of +0.0 and -0.0, every d2 the bits of +0, the lowest index wins."""
    src, tgt = K.denormal(name)
    d2, dsrc, dtgt = R.d2_matrix(src, tgt), _dev(api, ctx, src), _dev(api, ctx, tgt)
    for k in (1, 4, 16):
        idx, dist = _check_knn(api, ctx, src, tgt, k, d2, dsrc, dtgt, "denormal " + name)
        if name == "zeros":
            assert (idx == np.arange(k)).all() and (dist.view(np.uint32) == 0).all()
        else:
            assert (dist[:, 0] > 0).all() and (dist[:, 0] < K.FLT_MIN).mean() > 0.9
    sv, tv = R.valid_rows(src), R.valid_rows(tgt)
    fwd, rec = _check_lists(dsrc, dtgt, d2, sv, tv, None, "denormal " + name)
    assert len(fwd) == len(src) and 0 < len(rec) <= len(fwd)
    middle = float(np.sqrt(np.float64(np.median(fwd["distance"]))))           # a bound among the denormals: the compare is in double
    part, _ = _check_lists(dsrc, dtgt, d2, sv, tv, middle, "denormal " + name)
    assert (0 < len(part) < len(fwd)) or name == "zeros"


@pytest.mark.parametrize("k", [4, 16])
def test_source_is_target_past_the_first(api, ctx, k):
    """One cloud in both roles -- one validity array serves both -- at k > 1, on rows with copies and three invalid rows: column 0 is
    the lowest valid copy at d2 = 0, and the copies of a row come before every other row, in index order."""
    rows = K.self_rows()
    valid = R.valid_rows(rows)
    dc = _dev(api, ctx, rows)
    idx, dist = _check_knn(api, ctx, rows, rows, k, _self_d2(), dc, dc, "source is target")
    _, inverse = np.unique(rows, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.lexsort((np.arange(len(rows)), inverse))
    order = order[valid[order]]                                                # the valid rows, grouped by distinct row, ascending index inside
    starts = np.flatnonzero(np.r_[True, np.diff(inverse[order]) != 0])
    several = 0
    for a, b in zip(starts, np.r_[starts[1:], len(order)]):
        same = order[a:b]
        m = min(len(same), k)
        assert (idx[same, :m] == same[:m]).all() and (dist[same, :m] == 0).all() and (m == k or (dist[same, m] > 0).all())
        several += len(same) if len(same) > 1 else 0
    assert several > 100 and (idx[~valid] == -1).all() and (dist[~valid] == 0).all()


@functools.lru_cache(maxsize=None)
def _self_d2():
    rows = K.self_rows()
    return R.d2_matrix(rows, rows)


def test_capacity_smaller_than_found(api, ctx):
    from rsreg_amd import lib
    src, tgt = K.order()
    dsrc, dtgt = _prefix(api, ctx, "order", 0, len(src)), _prefix(api, ctx, "order", 1, len(tgt))
    full = dsrc.feature_correspondences(dtgt)
    out = np.full(40, 7, api.CORRESPONDENCE_DTYPE)
    found = C.c_size_t(0)
    lib.check(lib.lib().rsreg_cloud_feature_correspondences(ctx.h, dsrc.h, dtgt.h, R.DBL_MAX, 0, out.ctypes.data, 25, C.byref(found)), ctx.h)
    assert found.value == len(full) == len(src) and found.value > 25                  # nothing is hidden
    assert out[:25].tobytes() == full[:25].tobytes() and (out[25:]["index_query"] == 7).all()
    lib.check(lib.lib().rsreg_cloud_feature_correspondences(ctx.h, dsrc.h, dtgt.h, R.DBL_MAX, 1, None, 0, C.byref(found)), ctx.h)
    assert found.value == len(dsrc.feature_correspondences(dtgt, reciprocal=True))     # capacity 0: the count alone


def test_source_is_target(api, ctx):
    """Every valid row matches the lowest-indexed copy of itself at d2 = 0; the reciprocal list is exactly the rows that ARE that
    lowest copy."""
    rows = K.real()[1].copy()
    rows[[5, 1000, 2899], [0, 32, 7]] = [np.nan, np.inf, -np.inf]
    valid = R.valid_rows(rows)
    _, first, inverse = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    order = np.full(len(first), len(rows))
    np.minimum.at(order, inverse.reshape(-1)[valid], np.flatnonzero(valid))           # the lowest VALID row of each distinct row
    lowest = order[inverse.reshape(-1)]
    dc = _dev(api, ctx, rows)
    idx, dist = dc.feature_knn(dc, 1)
    assert (idx[valid, 0] == lowest[valid]).all() and (dist == 0).all() and (idx[~valid] == -1).all()
    assert (lowest[valid] != np.flatnonzero(valid)).sum() > 100                       # (copies exist, or this shows nothing)
    fwd = dc.feature_correspondences(dc)
    assert (fwd["index_query"] == np.flatnonzero(valid)).all() and (fwd["index_match"] == lowest[valid]).all() and (fwd["distance"] == 0).all()
    rec = dc.feature_correspondences(dc, reciprocal=True)
    own = np.flatnonzero(valid & (lowest == np.arange(len(rows))))
    assert (rec["index_query"] == own).all() and (rec["index_match"] == own).all()
    d2 = R.d2_matrix(rows, rows)
    _check_lists(dc, dc, d2, valid, valid, None, "source is target")


def test_determinism(api, ctx):
    """A second call, a fresh context that first matched clouds of other sizes, and api.CorrespondenceEstimation from host clouds and
    from device clouds: the same bytes."""
    src, tgt = K.real()
    dsrc, dtgt = _prefix(api, ctx, "real", 0, len(src)), _prefix(api, ctx, "real", 1, len(tgt))

    def everything(s, t):
        idx, dist = s.feature_knn(t, 5)
        return idx.tobytes(), dist.tobytes(), s.feature_correspondences(t).tobytes(), s.feature_correspondences(t, 40.0, True).tobytes()
    first = everything(dsrc, dtgt)
    assert everything(dsrc, dtgt) == first
    other = api.Context(0)
    a, b = _dev(api, other, K.order_rows(70, 1)), _dev(api, other, K.order_rows(9000, 2))
    a.feature_knn(b, 16)
    a.feature_correspondences(b, reciprocal=True)
    assert everything(_dev(api, other, src, 144, 3), _dev(api, other, tgt, 160, 4)) == first
    for s, t in ((dsrc, dtgt), (_host(api, src), _host(api, tgt)), (_host(api, src), dtgt), (dsrc, _host(api, tgt))):
        ce = api.CorrespondenceEstimation()
        ce.setInputSource(s)
        ce.setInputTarget(t)
        assert ce.determineCorrespondences().tobytes() == first[2]
        assert ce.determineReciprocalCorrespondences(40.0).tobytes() == first[3]
        assert ce.determineReciprocalCorrespondences().tobytes() == dsrc.feature_correspondences(dtgt, reciprocal=True).tobytes()


def test_end_to_end_on_the_device(api, ctx):
    """VoxelGrid -> normals_cloud(10) -> fpfh_cloud(k = 10) on two rendered frames, then both calls on the descriptors in HBM, equal
    to the reference run on the downloaded rows.  Printed, not asserted (nobody has measured it): the share of reciprocal matches
    that lie within 2 leaves of the ground-truth motion."""
    from rsreg_amd import synth
    leaf = 0.08
    clouds = []
    for frame in (0, 4):
        dc = api.DeviceCloud(synth.render_frame(frame, "50k", preset="bench"), ctx=ctx)
        vg = dc.voxel_grid(leaf)
        fc = vg.fpfh_cloud(vg.normals_cloud(10), 10)
        pts = vg.download().points
        clouds.append((np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float64), fc, fc.download_fpfh().points["histogram"]))
    (sxyz, sfc, srows), (txyz, tfc, trows) = clouds
    assert 500 < len(srows) < 6000 and 500 < len(trows) < 6000
    d2 = R.d2_matrix(srows, trows)
    sv, tv = R.valid_rows(srows), R.valid_rows(trows)
    for k in (1, 10):
        _check_knn(api, ctx, srows, trows, k, d2, sfc, tfc, "end to end")
    fwd, rec = _check_lists(sfc, tfc, d2, sv, tv, None, "end to end")
    T = synth.ground_truth(0, 4, "bench")
    moved = sxyz @ T[:3, :3].T + T[:3, 3]
    for name, lst in (("forward", fwd), ("reciprocal", rec)):
        err = np.linalg.norm(moved[lst["index_query"]] - txyz[lst["index_match"]], axis=1)
        print("end to end: %d x %d descriptors (%d, %d valid), %s matches %d, within 2 leaves of the true motion %.1f %%" %
              (len(srows), len(trows), sv.sum(), tv.sum(), name, len(lst), 100.0 * (err <= 2 * leaf).mean() if len(lst) else 0.0))


def test_refusals(api, ctx):
    """Every refusal of the contract: RSREG_ERR_INVALID_ARG, the outputs untouched."""
    from rsreg_amd import lib
    L, inv = lib.lib(), lib.RSREG_ERR_INVALID_ARG
    src, tgt = K.order_rows(40, 1), K.order_rows(30, 2)
    dsrc, dtgt = _dev(api, ctx, src), _dev(api, ctx, tgt)
    idx, dist = np.full((40, 16), 7, np.int32), np.full((40, 16), 7, np.float32)
    out, found = np.full(40, 7, api.CORRESPONDENCE_DTYPE), C.c_size_t(99)
    stamps = (dsrc.stamp, dtgt.stamp)

    def knn(s, t, k):
        return L.rsreg_cloud_feature_knn(ctx.h, s, t, k, idx.ctypes.data, dist.ctypes.data)

    def corr(s, t, max_distance=1.0, reciprocal=0, capacity=40, n_out=C.byref(found), host=out.ctypes.data):
        return L.rsreg_cloud_feature_correspondences(ctx.h, s, t, max_distance, reciprocal, host, capacity, n_out)
    assert knn(dsrc.h, dtgt.h, 0) == inv and knn(dsrc.h, dtgt.h, 17) == inv and knn(dsrc.h, dtgt.h, -1) == inv       # k out of range
    assert knn(None, dtgt.h, 1) == inv and knn(dsrc.h, None, 1) == inv                                                  # a NULL cloud
    assert corr(None, dtgt.h) == inv and corr(dsrc.h, None) == inv
    other = api.Context(0)
    foreign = _dev(api, other, tgt)
    assert knn(dsrc.h, foreign.h, 1) == inv and knn(foreign.h, dsrc.h, 1) == inv                                        # another context
    assert corr(dsrc.h, foreign.h) == inv and corr(foreign.h, dtgt.h) == inv
    narrow = api.DeviceCloud(api.FPFHCloud(np.zeros(30, np.dtype((np.void, 128))), 30, 1, True), ctx=ctx)               # a stride under 132
    assert knn(dsrc.h, narrow.h, 1) == inv and knn(narrow.h, dtgt.h, 1) == inv and corr(dsrc.h, narrow.h) == inv and corr(narrow.h, dtgt.h) == inv
    empty = _dev(api, ctx, src[:0])
    assert empty.info()[:2] == (0, 132) and knn(empty.h, dtgt.h, 1) == inv                                              # an empty source
    short, few = _dev(api, ctx, tgt[:15]), _dev(api, ctx, K.few_valid(4))
    assert knn(dsrc.h, dtgt.h, 16) == 0 and knn(dsrc.h, short.h, 16) == inv                                             # nt = k - 1
    idx[:], dist[:] = 7, 7
    assert knn(dsrc.h, few.h, 5) == inv                                                                                 # k - 1 valid rows of 70
    assert corr(dsrc.h, dtgt.h, -1.0) == inv and corr(dsrc.h, dtgt.h, float("nan")) == inv and corr(dsrc.h, dtgt.h, -0.5, 1) == inv
    assert corr(dsrc.h, dtgt.h, n_out=None) == inv and corr(dsrc.h, dtgt.h, host=None) == inv
    assert (idx == 7).all() and (dist == 7).all() and (out["index_query"] == 7).all() and (out["distance"] == 7).all() and found.value == 99
    assert (dsrc.stamp, dtgt.stamp) == stamps
    # not refusals: no valid row on either side, an empty cloud -- nothing found
    nothing = _dev(api, ctx, np.full((20, 33), np.nan, np.float32))
    assert corr(dsrc.h, nothing.h) == 0 and found.value == 0
    found.value = 99
    assert corr(nothing.h, dtgt.h, 1.0, 1) == 0 and found.value == 0
    found.value = 99
    assert corr(empty.h, dtgt.h) == 0 and found.value == 0 and (out["index_query"] == 7).all()
    with pytest.raises(lib.RsregError) as e:
        dsrc.feature_knn(dtgt, 17)
    assert e.value.status == inv and "between 1 and 16" in str(e.value)
    with pytest.raises(lib.RsregError) as e:
        dsrc.feature_correspondences(dtgt, -1.0)
    assert e.value.status == inv
    assert L.rsreg_version() == 4


def test_cpp_adaptor(api, ctx, tmp_path):
    """tests/cpp/feature_match_runner.cpp (rsreg::registration::CorrespondenceEstimation) gives the bytes of the Python path, from
    host clouds and from device clouds, at the default max_distance and at a finite one."""
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "feature_match_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "feature_match_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    src, tgt = K.holes()
    dsrc, dtgt = _dev(api, ctx, src), _dev(api, ctx, tgt)
    K.records(src).tofile(str(tmp_path / "source.bin"))
    K.records(tgt).tofile(str(tmp_path / "target.bin"))
    for arg, md in (("max", None), ("40.5", 40.5)):
        prefix = str(tmp_path / ("run_%s_" % arg))
        r = subprocess.run([exe, str(tmp_path / "source.bin"), str(tmp_path / "target.bin"), arg, prefix], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout
        vals = dict(l.split() for l in r.stdout.strip().splitlines())
        fwd, rec = dsrc.feature_correspondences(dtgt, md), dsrc.feature_correspondences(dtgt, md, True)
        assert len(fwd) > len(rec) > 0
        for name, want in (("fwd_host", fwd), ("rec_host", rec), ("fwd_device", fwd), ("rec_device", rec)):
            assert open(prefix + name + ".bin", "rb").read() == want.tobytes() and int(vals[name]) == len(want)
