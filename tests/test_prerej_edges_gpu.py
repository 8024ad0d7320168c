"""rsreg_cloud_score_transforms and rsreg_cloud_prerejective on the GPU at the cases of tests/prerej_edge_cases.py, against
tests/prerej_ref.py: second and later rounds of hypotheses, transforms scored past a round, a source of 8 193 tiles (a batch of 255),
degenerate samples (the polygon test's 0 / 0, 0 / x and inf / inf, the rank-deficient solve as the hypothesis kernel builds it), both
clouds times 2^e (the division of float32 denormals), a range AT a float d2, a cloud at 2^62 thrown out of the float range.

Everything is EQUAL to the reference, as in tests/test_prerej_gpu.py (whose _same_result and _same_scores compare here): there is no
tolerance.  tests/test_prerej_edges_cpu.py proves on the reference that each case reaches the branch it is named for.

Measured on one MI355X: the file 4.2 s, its slowest test (the three-round case, its reference included) 0.8 s.
"""
import numpy as np
import pytest

import prerej_cases as C
import prerej_edge_cases as X
import prerej_ref as R
from test_prerej_gpu import _dev, _same_result, _same_scores

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


def _stage_scores(api, dsrc, dtgt, name, want, hypotheses):
    """the counts and sums of the valid hypotheses `hypotheses` of a case, through the scoring stage on its own"""
    src, tgt, nbr, prm = X.CASES[name]
    if not len(hypotheses):
        return
    Ts = np.array([R.hypothesis(api, R.xyz_of(src), R.xyz_of(tgt), nbr, prm["seed"], int(h), prm.get("similarity_threshold", 0.9))[0] for h in hypotheses])
    _same_scores(dsrc.score_transforms(dtgt, Ts, prm["max_correspondence_distance"]), (want.counts[hypotheses], want.sums[hypotheses]), name)


@pytest.mark.parametrize("name", list(X.CASES))
def test_prerejective_edge_case_equals_the_reference(api, ctx, name):
    src, tgt, nbr, prm = X.CASES[name]
    want = X.reference(name)
    dsrc = _dev(api, ctx, src, 32)
    dtgt = dsrc if name in X.SAME_CLOUD else _dev(api, ctx, tgt, 16, 1)
    inliers, got = dsrc.prerejective(dtgt, nbr, **prm)
    _same_result(inliers, got, want, name)
    if not want.found:
        assert (got.transform == np.eye(4)).all() and got.n_inliers == 0 and got.fitness == 0.0 and len(inliers) == 0
        assert got.best_hypothesis == -1 and tuple(got.sample) == tuple(got.match) == (-1, -1, -1)
    # the first 40 valid hypotheses of EVERY round through the scoring stage: the valid flag of each (n_valid above counts them), its
    # transform's count and its sum
    valid = np.flatnonzero(want.valid)
    for r0 in range(0, prm["max_iterations"], X.ROUND):
        _stage_scores(api, dsrc, dtgt, name, want, valid[(valid >= r0) & (valid < r0 + X.ROUND)][:40])


def test_score_transforms_past_a_round(api, ctx):
    src, tgt, Ts, pick, rng = X.score_past_a_round()
    counts, sums = X.distinct_scores("past_a_round")
    _same_scores(_dev(api, ctx, src).score_transforms(_dev(api, ctx, tgt, seed=1), Ts[pick], rng), (counts[pick], sums[pick]), "past a round")


def test_score_transforms_under_a_batch_cap_below_256(api, ctx):
    src, tgt, Ts, pick, rng = X.batch_cap_below_256()
    counts, sums = X.distinct_scores("cap")
    assert C.batch_cap(len(src)) == 255 < len(pick)
    _same_scores(_dev(api, ctx, src, 12).score_transforms(_dev(api, ctx, tgt, seed=1), Ts[pick], rng), (counts[pick], sums[pick]), "batch cap")


def test_range_at_a_float(api, ctx):
    """one source record, one or two target records, the identity: a range whose square is AT the float d2, one double above, one
    below; 0, and ranges whose square is 0, below 2^-149, above FLT_MAX and +inf"""
    eye = np.eye(4, dtype=np.float32)
    for label, s, t, d2 in X.range_pairs():
        dsrc, dtgt = _dev(api, ctx, s), _dev(api, ctx, t, seed=1)
        ranges = list(X.FIXED_RANGES)
        if np.isfinite(d2):
            out, inside = X.ranges_around(d2)
            ranges += out + inside
        for rng in ranges:
            inlier = float(d2) < rng * rng
            want = (np.array([int(inlier)], np.uint32), np.array([float(d2) if inlier else 0.0]))
            assert R.score(eye, s, t, rng)[:2] == (want[0][0], want[1][0])
            _same_scores(dsrc.score_transforms(dtgt, eye, rng), want, (label, rng))


def test_score_transforms_of_a_cloud_thrown_out_of_range(api, ctx):
    src, tgt, Ts = X.thrown_out_of_range()
    dsrc, dtgt = _dev(api, ctx, src), _dev(api, ctx, tgt, seed=1)
    for rng in X.THROWN_RANGES:
        _same_scores(dsrc.score_transforms(dtgt, Ts, rng), R.score_transforms(Ts, src, tgt, rng), rng)
