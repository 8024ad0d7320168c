"""GPU: the running best of the dense-table search is one 64-bit key, d_bits << 32 | index, held as an IEEE double and
updated with one f64 minimum per candidate (csrc/icp_dense.hpp: DBest).  The cases where that could differ from the
unsigned 64-bit compare it stands for: a zero distance (the key is then a subnormal double), exact ties (the low word
decides), nothing found (the start value, +inf | 0xffffffff) and a squared distance that overflows to +inf.

Every case goes through the staged search (unseeded, then seeded by its own result) against a float32 brute force that
follows FLANN's L2_Simple order with the lowest-index tie-break, and through the fused kernels -- pipelines 1 and 2,
unsplit and with every tile split over 2 / over 2 and 4 lanes per query:
  * three iterations (the second and third seeded): the same bits as the staged pipeline;
  * one iteration (unseeded; for the split forms under the schedule carried over from the three-iteration alignment, so the
    first launch is split too): the number of matches, the sum of the matched target points and the sum of the squared
    distances, against the brute force's matches.  These are f64 sums of n <= 4096 terms added up in another order than
    numpy's, so each may differ by n * 2^-53 * sum(|terms|) at the most; on the lattice scene the coordinates are
    small multiples of 2^-8 and the sums of the target points are exact: a tie that went to the wrong index shows there."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GATES = [0.013, 1e30]
SCHED_KEYS = ("RSREG_SCHED", "RSREG_SCHED_MIN_TILES", "RSREG_SCHED_F2", "RSREG_SCHED_F4", "RSREG_SCHED_AT")
SPLIT2 = {"RSREG_SCHED": "1", "RSREG_SCHED_MIN_TILES": "1", "RSREG_SCHED_F2": "1.0", "RSREG_SCHED_F4": "0.0"}
SPLIT24 = {"RSREG_SCHED": "1", "RSREG_SCHED_MIN_TILES": "1", "RSREG_SCHED_F2": "0.5", "RSREG_SCHED_F4": "0.5"}
UNSPLIT = {"RSREG_SCHED": "0"}


@pytest.fixture(scope="module")
def api(rs):
    from rsreg_amd import api as a, lib
    lib.build()
    if a.device_count() < 1:
        pytest.fail("no HIP device: the product has no CPU fallback")
    return a


def brute(src, tgt, gate):
    """tests/test_nn_fuzz_gpu.py's brute force: float32, (dx^2 + dy^2) + dz^2, first minimum, PCL's gate in double."""
    s = src.astype(np.float32)
    t = tgt.astype(np.float32)
    idx = np.full(len(s), -1, np.int64)
    d2o = np.zeros(len(s), np.float32)
    ok_t = np.isfinite(t).all(1)
    ti = np.nonzero(ok_t)[0]
    tt = t[ok_t]
    gate2 = float(gate) * float(gate)
    with np.errstate(over="ignore"):
        for i in range(len(s)):
            if not np.isfinite(s[i]).all() or len(tt) == 0:
                continue
            d = s[i] - tt
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]   # float32, FLANN's order
            j = int(np.argmin(d2))                                             # first minimum = lowest index
            if not (float(d2[j]) > gate2):
                idx[i] = ti[j]
                d2o[i] = d2[j]
    return idx, d2o


def _set_env(monkeypatch, env):
    for k in SCHED_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _result(icp, out):
    r = icp.result
    return (bytes(r.transform), bytes(r.sums_last), r.n_correspondences, r.iterations, r.state, r.converged, r.mse,
            np.stack([out.points[k] for k in "xyz"]).tobytes())


def check_all_forms(api, rs, monkeypatch, src, tgt, gate, want_dense=False):
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    want_idx, want_d2 = brute(src, tgt, gate)
    hit = want_idx >= 0
    sc, tc = rs.PointCloud.from_xyz(src), rs.PointCloud.from_xyz(tgt)

    def new_icp(pipeline, iters):
        icp = api.IterativeClosestPoint(api.Context(0))
        icp.params = api.icp_params(max_iterations=iters, criteria_mode=1, pipeline_mode=pipeline, max_correspondence_distance=gate)
        icp.setInputSource(sc)
        icp.setInputTarget(tc)
        return icp

    # ---- the staged search: unseeded, then seeded
    _set_env(monkeypatch, UNSPLIT)
    icp = new_icp(0, 3)
    icp.begin()
    for seeded in (False, True):
        idx, d2 = icp.search()
        assert np.array_equal(idx.astype(np.int64), want_idx), ("staged", seeded, gate)
        assert np.array_equal(d2[hit], want_d2[hit]), ("staged", seeded, gate)
    if want_dense and not os.environ.get("RSREG_FORCE_HASH") and not os.environ.get("RSREG_DENSE_MAX_CELLS"):
        assert icp.grid_info().index_kind == 1   # the dense table: the index whose search keeps the key
    icp.end()
    staged3 = _result(icp, icp.align())

    # ---- what one iteration's 17 sums must hold (a[0] matches, a[4..6] their target points, a[16] their squared distances)
    n = len(src)
    t64, d64 = tgt[want_idx[hit]].astype(np.float64), want_d2[hit].astype(np.float64)
    finite_d = bool(np.isfinite(d64).all())
    want_q, want_d = t64.sum(0), d64.sum()
    tol_q, tol_d = n * 2.0 ** -53 * np.abs(t64).sum(0), n * 2.0 ** -53 * np.abs(d64).sum()

    # ---- the fused kernels
    for name, pipeline, env in (("fused 1", 1, UNSPLIT), ("fused 2", 2, UNSPLIT), ("split by 2", 2, SPLIT2), ("split by 2 and 4", 2, SPLIT24)):
        _set_env(monkeypatch, env)
        icp = new_icp(pipeline, 3)
        got3 = _result(icp, icp.align())
        split = env is not UNSPLIT
        if split:
            assert icp.result.n_scheduled_launches > 0, (name, "the schedule was not built")
        assert got3 == staged3, (name, gate)
        icp.params = api.icp_params(max_iterations=1, criteria_mode=1, pipeline_mode=pipeline, max_correspondence_distance=gate)
        icp.align()
        r = icp.result
        if split:
            assert r.n_scheduled_launches == r.n_nn_launches, (name, "the first launch ran unsplit")
        sums = np.array(r.sums_last, np.float64)
        print("%s gate %g: matches %d (want %d), |dQ| %s (bound %s), dD %.3g (bound %.3g)" %
              (name, gate, r.n_correspondences, int(hit.sum()), np.abs(sums[4:7] - want_q), tol_q, abs(sums[16] - want_d) if finite_d else 0.0, tol_d if finite_d else 0.0))
        assert r.n_correspondences == int(hit.sum()), (name, gate)
        assert sums[0] == float(hit.sum()), (name, gate)
        assert (np.abs(sums[4:7] - want_q) <= tol_q).all(), (name, gate)
        if finite_d:
            assert abs(sums[16] - want_d) <= tol_d, (name, gate)
        else:
            assert sums[16] == want_d, (name, gate)   # (+inf)
    return want_idx, want_d2


@pytest.mark.parametrize("gate", GATES)
def test_zero_distance(api, rs, monkeypatch, gate):
    """Queries that coincide exactly with target points: d^2 = 0, the key is index alone -- a subnormal double, or +0.0 for
    the one query on target point 0."""
    rng = np.random.default_rng(41)
    tgt = rng.uniform(-0.3, 0.3, (3000, 3)).astype(np.float32)
    pick = np.concatenate([1 + rng.permutation(2999)[:900], [0]])
    src = tgt[pick].copy()
    idx, d2 = check_all_forms(api, rs, monkeypatch, src, tgt, gate, want_dense=True)
    assert np.array_equal(idx, pick) and not d2.any()


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("gate", GATES)
def test_exact_ties(api, rs, monkeypatch, gate, reverse):
    """The lattice scene of the fuzz test (points on a 2^-7 grid, many of them several times) and queries half a step off
    it in x, in x and y, or in all three: 2, 4 or 8 lattice sites -- and every copy of a point on them -- are exactly as far.
    The lowest original index wins, whichever way round the target is indexed."""
    from test_nn_fuzz_gpu import scene
    rng = np.random.default_rng(42)
    tgt = scene(rng, "lattice", 3000).astype(np.float32)
    if reverse:
        tgt = tgt[::-1].copy()
    src = scene(rng, "lattice", 1000)
    off = np.zeros((1000, 3))
    off[:, 0] = 0.00390625
    off[333:, 1] = 0.00390625
    off[666:, 2] = 0.00390625
    src = (src + off).astype(np.float32)
    idx, d2 = check_all_forms(api, rs, monkeypatch, src, tgt, gate, want_dense=True)
    # (the scene does what it is for: most queries have more than one nearest point)
    t = tgt.astype(np.float32)
    ties = 0
    for i in range(0, 1000, 10):
        d = src[i] - t
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ties += int((dd == dd.min()).sum() > 1)
    assert ties > 50


@pytest.mark.parametrize("gate", GATES)
def test_beyond_the_gate_and_one_point_target(api, rs, monkeypatch, gate):
    """Queries with nothing inside the gate keep the start value (+inf, no point) and give -1; a target of one point."""
    rng = np.random.default_rng(43)
    tgt = rng.uniform(-0.2, 0.2, (500, 3)).astype(np.float32)
    near = tgt[rng.permutation(500)[:300]] + rng.normal(0, 0.002, (300, 3)).astype(np.float32)
    far = rng.uniform(-0.2, 0.2, (300, 3)).astype(np.float32) + np.array([1.5, -2.0, 0.7], np.float32)
    idx, _ = check_all_forms(api, rs, monkeypatch, np.concatenate([near, far]), tgt, gate)
    if gate < 1.0:
        assert (idx[300:] == -1).all() and (idx[:300] >= 0).any()
    one = np.array([[0.05, -0.02, 0.3]], np.float32)
    src = np.concatenate([one + rng.normal(0, 0.004, (200, 3)), one + rng.uniform(0.5, 1.0, (200, 3))]).astype(np.float32)
    idx, _ = check_all_forms(api, rs, monkeypatch, src, one, gate)
    if gate < 1.0:
        assert (idx[200:] == -1).all() and (idx[:200] == 0).any()


@pytest.mark.parametrize("gate", GATES)
def test_squared_distance_overflows(api, rs, monkeypatch, gate):
    """Finite queries 10^20 away from a finite target: d^2 = 10^40 is +inf in float32, the key's high word that of the start
    value.  The same answer as the brute force (PCL's gate: inf > gate^2, no match), next to ordinary queries."""
    rng = np.random.default_rng(44)
    tgt = rng.uniform(-0.2, 0.2, (800, 3)).astype(np.float32)
    near = tgt[rng.permutation(800)[:300]] + rng.normal(0, 0.002, (300, 3)).astype(np.float32)
    far = np.zeros((100, 3), np.float32)
    far[np.arange(100), rng.integers(0, 3, 100)] = 1e20
    far[::2] *= -1
    far += rng.uniform(-0.1, 0.1, (100, 3)).astype(np.float32)
    src = np.concatenate([near, far])
    with np.errstate(over="ignore"):
        assert np.isinf(((src[300:, None, :] - tgt[None, :8, :]) ** 2).sum(-1)).all()
    idx, _ = check_all_forms(api, rs, monkeypatch, src, tgt, gate)
    assert (idx[300:] == -1).all()
