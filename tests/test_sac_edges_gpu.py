"""The pose-from-correspondences entry points on the GPU at the cases of tests/sac_edge_cases.py, against tests/sac_ref.py: degenerate
three-pair samples (the rank-deficient solve as sac.hip builds it for the device), the edges of the stopping rule, every capacity
around the number kept, a list of 70 001 pairs, the float32 range and thresholds whose square is not an ordinary float.

Everything is EQUAL to the reference, as in tests/test_sac_gpu.py: found, best_hypothesis, sample, iterations, n_inliers, n_out,
the kept bytes, and -- without a refit -- all 16 floats of the transform.  tests/test_sac_edges_cpu.py proves on the reference that
each case reaches the branch it is named for.
"""
import functools
import math

import numpy as np
import pytest

import sac_cases as K
import sac_edge_cases as E
import sac_ref as R
from test_sac_gpu import _check_counts, _dev, _same_result

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


def _sums_within_the_tree_bound(sums, P, Q, finite):
    """tests/test_sac_gpu.py's bound: m * 2^-53 * sum|terms| around math.fsum of the exact terms, m = sac_ref.sum_tree_depth(n).  (A
    sum with a term of +inf -- a float32 d2 that overflowed -- is +inf.)"""
    terms = R.exact_terms(P, Q, finite)
    m = R.sum_tree_depth(len(P))
    assert sums[0] == finite.sum()
    for k in range(R.NUM_SUMS):
        if np.isinf(terms[k]).any():
            assert (terms[k] > -np.inf).all() and sums[k] == np.inf, (k, sums[k])
            continue
        exact, bound = math.fsum(terms[k]), m * 2.0 ** -53 * math.fsum(np.abs(terms[k]))
        assert abs(sums[k] - exact) <= bound, (k, sums[k], exact, bound)


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_sac_edge_case_equals_the_reference(api, ctx, name):
    want, src, tgt, corr, true, prm = E.reference(name)
    dsrc, dtgt = _dev(api, ctx, src, 32), _dev(api, ctx, tgt, 16, 1)
    kept, got = dsrc.sac_correspondences(dtgt, corr, **prm)
    _same_result(kept, got, want)
    n = len(corr)
    if want.found:
        # every capacity around the number kept: the first `capacity` records, the full number reported, nothing else changes
        for room in E.capacities(got.n_inliers):
            few, again = dsrc.sac_correspondences(dtgt, corr, capacity=room, **prm)
            assert again.n_out == got.n_inliers == again.n_inliers and len(few) == min(room, got.n_inliers), (name, room)
            assert few.tobytes() == kept[:room].tobytes() and again.transform.tobytes() == got.transform.tobytes(), (name, room)
            assert (again.found, again.best_hypothesis, tuple(again.sample), again.iterations) == (got.found, got.best_hypothesis, tuple(got.sample), got.iterations)
    else:
        assert not got.found and (got.transform == np.eye(4)).all() and kept.tobytes() == corr.tobytes() and got.n_inliers == 0
        assert got.best_hypothesis == -1 and tuple(got.sample) == (-1, -1, -1)
        for room in (0, 1, n - 1, n + 1):                                        # NO MODEL: the input list, cut to the capacity
            few, again = dsrc.sac_correspondences(dtgt, corr, capacity=room, **prm)
            assert again.n_out == n and few.tobytes() == corr[:room].tobytes() and not again.found and again.iterations == got.iterations
    # the case's list through the two other entry points: the winner's transform, the identity, MOTION and thirteen near it at the
    # case's threshold; the SVD fit over the whole list
    Ts = np.concatenate([np.stack([np.asarray(want.transform, np.float32), np.eye(4, dtype=np.float32), K.MOTION.astype(np.float32)]), K.transforms(13, 3)])
    counts = _check_counts(api, ctx, src, tgt, corr, Ts, prm.get("inlier_threshold", 0.05), dsrc, dtgt, label=name)
    if want.found:
        assert counts[0] == want.n_inliers
    T, sums = dsrc.estimate_rigid_svd(dtgt, corr)
    assert T.tobytes() == api.umeyama_from_sums(sums).tobytes()
    P, Q, finite = R.pair_points(src, tgt, corr)
    _sums_within_the_tree_bound(sums, P, Q, finite)
    if name in ("collinear", "collinear_exact_turn"):                            # every pair a true pair of one motion: the fit maps the line onto its image
        assert np.abs(P.astype(np.float64) @ T[:3, :3].T.astype(np.float64) + T[:3, 3] - Q).max() < 1e-4


def test_probability_next_to_one_is_refused(api, ctx):
    """(0, 1) is open: 1 - 2^-54 is not a double and rounds to 1.0, refused; the largest double below 1 runs (a case above)"""
    from rsreg_amd import lib as L
    want, src, tgt, corr, true, prm = E.reference("all_inliers")
    dsrc, dtgt = _dev(api, ctx, src), _dev(api, ctx, tgt, seed=1)
    for p in (1.0 - 2.0 ** -54, 1.0, 0.0, -0.0, math.nan):
        with pytest.raises(L.RsregError) as e:
            dsrc.sac_correspondences(dtgt, corr, probability=p)
        assert e.value.status == L.RSREG_ERR_INVALID_ARG
    kept, got = dsrc.sac_correspondences(dtgt, corr, probability=5e-324, seed=111)            # the least positive double: log(1 - p) is 0
    assert got.found and got.iterations == 1


@functools.lru_cache(maxsize=None)
def _big_counts():
    """the reference's counts of the 331 distinct transforms against the first EXACT_N, EXACT_N + 1 and all BIG_N pairs"""
    src, tgt, corr, true = E.big()
    P, Q, finite = R.pair_points(src, tgt, corr)
    base, pick = E.transforms_fast_pick(E.BIG_H)
    cum = np.zeros((len(base), 3), np.uint32)
    for a in range(0, len(base), 32):
        f = R.within(base[a:a + 32], P, Q, finite, 0.05)
        cum[a:a + 32] = np.stack([f[:, :E.EXACT_N].sum(axis=1), f[:, :E.EXACT_N + 1].sum(axis=1), f.sum(axis=1)], axis=1)
    return base, pick, cum


_BIG = {}


def _big_clouds(api, ctx):
    if "big" not in _BIG:
        src, tgt, corr, true = E.big()
        _BIG["big"] = (_dev(api, ctx, src), _dev(api, ctx, tgt, seed=1))
    return _BIG["big"]


@pytest.mark.parametrize("which, n", ((0, E.EXACT_N), (1, E.EXACT_N + 1), (2, E.BIG_N)))
def test_count_inliers_many_tiles_and_a_grown_slice(api, ctx, which, n):
    """4 096 transforms against 32 768 pairs (64 tiles x 64 chunks: MAX_GROUPS workgroups exactly, a slice is one chunk), against one
    pair more (a slice is two chunks) and against 70 001 pairs (137 tiles, slices of three chunks, the last one ragged)"""
    src, tgt, corr, true = E.big()
    dsrc, dtgt = _big_clouds(api, ctx)
    base, pick, cum = _big_counts()
    assert K.plan(n, E.BIG_H)[2] == (1, 2, 3)[which]
    got = dsrc.count_inliers(dtgt, corr[:n], base[pick], 0.05)
    want = cum[pick, which]
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (n, bad[:5], got[bad[:5]], want[bad[:5]])
    assert want.max() > 0.49 * n and (want == 0).sum() > 100


@pytest.mark.parametrize("name", ("big", "collinear_noisy", "one_target", "coplanar_mirrored", "scale_2^-62", "scale_2^+100"))
def test_refit_equals_the_reference(api, ctx, name):
    """refit_rounds 2, compared through the fit= hook as tests/test_sac_gpu.py does.  "big": 70 001 pairs -- the flags, the scan (69
    tiles of 1 024), the emit of 35 000 records, the refit's sums over 547 groups.  The others: a fit over collinear or coincident
    inliers, and over pairs whose d2 is a denormal or +inf."""
    want, src, tgt, corr, true, prm = E.reference(name)
    dsrc, dtgt = _big_clouds(api, ctx) if name == "big" else (_dev(api, ctx, src), _dev(api, ctx, tgt, seed=1))
    dnan = _dev(api, ctx, np.concatenate([src, np.full((1, 3), np.nan, np.float32)]))

    def fit(flags):
        masked = corr.copy()
        masked["index_query"][~flags] = len(src)
        return dnan.estimate_rigid_svd(dtgt, masked)

    ref2 = R.sac(api, src, tgt, corr, refit_rounds=2, counts=(want.counts, want.valid), fit=fit, **prm)
    kept2, got2 = dsrc.sac_correspondences(dtgt, corr, refit_rounds=2, **prm)
    _same_result(kept2, got2, ref2, refit=True)
    assert 1 <= got2.refit_rounds_run == ref2.refit_rounds_run
    assert got2.transform.tobytes() == ref2.transform.tobytes() and got2.sums.tobytes() == ref2.sums.tobytes()
    assert got2.transform.tobytes() == api.umeyama_from_sums(got2.sums).tobytes()
    if name == "big":
        assert np.linalg.norm(got2.transform.astype(np.float64) - K.MOTION) < 1e-4
    room = got2.n_inliers - 1
    few, again = dsrc.sac_correspondences(dtgt, corr, refit_rounds=2, capacity=room, **prm)
    assert again.n_out == got2.n_inliers and few.tobytes() == kept2[:room].tobytes()


def test_count_inliers_at_range_thresholds(api, ctx):
    """threshold^2 = +inf in double, above FLT_MAX, below the least denormal, 0: the least float >= threshold^2 is +inf, +inf, 2^-149,
    0, against pairs whose d2 is 0, 2^-149, 2^-148, just below FLT_MAX, +inf and NaN; and thresholds whose square is a float"""
    src, tgt, corr, d2 = E.range_threshold_pairs()
    dsrc, dtgt = _dev(api, ctx, src), _dev(api, ctx, tgt, seed=1)
    eye = np.eye(4, dtype=np.float32)[None]
    for thr, n_in in zip(E.RANGE_THRESHOLDS, (9, 9, 2, 0)):
        want = _check_counts(api, ctx, src, tgt, corr, eye, thr, dsrc, dtgt, label=thr)
        assert want[0] == n_in
    for thr in (2.0 ** -74, 2.0 ** -74.5, 1.8e19, 1.85e19):                       # between the pairs
        _check_counts(api, ctx, src, tgt, corr, eye, thr, dsrc, dtgt, label=thr)
    for thr in (0.5, 2.0 ** -10):
        src, tgt, corr, d2 = K.threshold_pairs(thr)
        want = _check_counts(api, ctx, src, tgt, corr, eye, thr, label=thr)
        assert want[0] == 8                                                      # d2 == threshold^2 is outside


def test_count_inliers_with_extreme_transforms(api, ctx):
    """FLT_MAX, denormals and -0.0 in the transforms, points near FLT_MAX: inf - inf on the way is a NaN and no inlier, an intermediate
    +inf never comes back finite, so every row's count is the reference's"""
    src, tgt, corr, Ts = E.extreme_transforms_case()
    dsrc, dtgt = _dev(api, ctx, src), _dev(api, ctx, tgt, seed=1)
    for thr in (E.RANGE_THRESHOLDS[0], 1e19, 0.05, 1e-30):
        _check_counts(api, ctx, src, tgt, corr, Ts, thr, dsrc, dtgt, label=thr)


def test_estimate_rigid_svd_with_few_finite_pairs(api, ctx):
    from rsreg_amd import lib as L
    src, tgt, corr, keep = E.few_finite_case(2)
    with pytest.raises(L.RsregError) as e:
        _dev(api, ctx, src).estimate_rigid_svd(_dev(api, ctx, tgt, seed=1), corr)
    assert e.value.status == L.RSREG_ERR_INVALID_ARG
    src, tgt, corr, keep = E.few_finite_case(3)
    T, sums = _dev(api, ctx, src).estimate_rigid_svd(_dev(api, ctx, tgt, seed=1), corr)
    assert sums[0] == 3 and T.tobytes() == api.umeyama_from_sums(sums).tobytes()
    P, Q, finite = R.pair_points(src, tgt, corr)
    assert (np.flatnonzero(finite) == keep).all()
    _sums_within_the_tree_bound(sums, P, Q, finite)
    assert np.abs(P[keep].astype(np.float64) @ T[:3, :3].T.astype(np.float64) + T[:3, 3] - Q[keep]).max() < 1e-5
