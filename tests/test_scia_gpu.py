"""rsreg_cloud_error_transforms, rsreg_cloud_initial_alignment_hypotheses and rsreg_cloud_initial_alignment
(pcl::SampleConsensusInitialAlignment: poses from descriptor neighbours, every one scored over every source record by a robust
error of its exact nearest-point distance) on the GPU and the Python adaptor, against tests/scia_ref.py on the cases of
tests/scia_cases.py.

Errors, transforms, flags, samples, the winner and every field of the result are EQUAL to the reference: the contract
(include/rsreg.h) fixes the generator, the operation order of a term, the order of the sum and the selection, so there is no
tolerance anywhere but in the recovery test, whose bar is the issue's.
"""
import math

import numpy as np
import pytest

import prerej_cases as C
import prerej_edge_cases as PE
import sac_cases as S
import scia_cases as K
import scia_ref as R

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


def _dev(api, ctx, xyz, stride=16, seed=0):
    return api.DeviceCloud(api.NormalCloud(S.records(xyz, stride, seed), len(xyz), 1, False), ctx=ctx)


def _same_errors(got, want, label):
    assert got.dtype == np.float64 and got.shape == want.shape, label
    bad = np.flatnonzero(got.view(np.uint64) != np.asarray(want, np.float64).view(np.uint64))
    assert len(bad) == 0, (label, bad[:5], got[bad[:5]], want[bad[:5]])


# ---- the scoring stage
@pytest.mark.parametrize("name", list(K.SCORE_CASES))
def test_error_transforms_equals_the_reference(api, ctx, name):
    src, tgt, Ts, fn, mcd = K.SCORE_CASES[name]
    _same_errors(_dev(api, ctx, src).error_transforms(_dev(api, ctx, tgt, seed=1), Ts, fn, mcd), K.score_reference(name), name)


@pytest.mark.parametrize("fn", (K.TRUNCATED, K.HUBER))
def test_error_transforms_one_float_step_around_thr(api, ctx, fn):
    """one source record whose e is exact (0 .. the largest float below 2^127, +inf) against thr one step below e, at e, one step
    above, 2^-149 and +inf"""
    eye = np.eye(4, dtype=np.float32)
    for label, s, t, e, thrs in K.step_pairs():
        ds, dt = _dev(api, ctx, s), _dev(api, ctx, t, seed=1)
        for thr in thrs:
            got = ds.error_transforms(dt, eye, fn, thr)
            want = R.error_transforms(eye[None], s, t, fn, thr)
            _same_errors(got, want, (label, thr))
            if fn == K.TRUNCATED and np.isfinite(e) and e > 0 and math.isfinite(thr):
                assert (got[0] < 1.0) == (float(e) < thr) and (got[0] == 1.0) == (float(e) >= thr), (label, thr, got)


def test_error_transforms_record_layouts_and_one_cloud(api, ctx):
    for name in ("truncated_source_129", "huber_source_129"):
        src, tgt, Ts, fn, mcd = K.SCORE_CASES[name]
        want = K.score_reference(name)
        for ss, ts in zip(C.STRIDES, reversed(C.STRIDES)):
            _same_errors(_dev(api, ctx, src, ss).error_transforms(_dev(api, ctx, tgt, ts, 1), Ts, fn, mcd), want, (name, ss, ts))
        # source == target: under the identity every finite record finds itself at e = 0
        one = _dev(api, ctx, tgt, 32)
        got = one.error_transforms(one, Ts, fn, mcd)
        _same_errors(got, R.error_transforms(Ts, tgt, tgt, fn, mcd), "one cloud")
        assert got[0] == 0.0 and not np.signbit(got[0])


def test_error_transforms_one_call_equals_one_call_each(api, ctx):
    name = "truncated_transforms_%d" % (C.MAX_BATCH + 1)
    src, tgt, Ts, fn, mcd = K.SCORE_CASES[name]
    dsrc, dtgt = _dev(api, ctx, src), _dev(api, ctx, tgt, seed=1)
    errors = dsrc.error_transforms(dtgt, Ts, fn, mcd)
    for h in list(range(14)) + [C.MAX_BATCH - 1, C.MAX_BATCH]:
        assert dsrc.error_transforms(dtgt, Ts[h], fn, mcd).view(np.uint64)[0] == errors.view(np.uint64)[h], h


def test_error_transforms_batch_capped_below_256(api, ctx):
    """a source of 8 193 tiles: 256 rows go out as a batch of 255 and a batch of 1, a hypothesis's partial sums lie 8 193 groups apart"""
    src, tgt, Ts, pick, rng = PE.batch_cap_below_256()
    got = _dev(api, ctx, src, 12).error_transforms(_dev(api, ctx, tgt, seed=1), Ts[pick], K.TRUNCATED, rng * rng)
    _same_errors(got, K.batch_cap_reference(), "batch cap")


# ---- the sampler and the fit
def _same_hypotheses(got, want, label):
    Ts, valid, words = got
    assert Ts.dtype == np.float32 and valid.dtype == bool and words.dtype == np.int32, label
    assert (valid == want[1]).all(), (label, np.flatnonzero(valid != want[1])[:5])
    assert words.tobytes() == want[2].tobytes(), (label, np.flatnonzero((words != want[2]).any(axis=1))[:5])
    assert np.isnan(Ts[~valid]).all(), label
    assert Ts[valid].tobytes() == want[0][want[1]].tobytes(), label
    assert (Ts[valid][:, 3] == np.float32([0, 0, 0, 1])).all(), label


@pytest.mark.parametrize("name", list(K.HYP_CASES))
def test_hypotheses_equal_the_reference(api, ctx, name):
    src, tgt, nbr, prm, count = K.HYP_CASES[name]
    want = K.hyp_reference(name)
    dsrc, dtgt = _dev(api, ctx, src, 32), _dev(api, ctx, tgt, 16, 1)
    _same_hypotheses(dsrc.initial_alignment_hypotheses(dtgt, nbr, 0, count, **prm), want, name)
    # first > 0: the same rows as from 0
    if count >= 32:
        first = count - 20
        tail = dsrc.initial_alignment_hypotheses(dtgt, nbr, first, 20, **prm)
        _same_hypotheses(tail, tuple(w[first:] for w in want), (name, first))


def test_hypotheses_past_a_round_and_at_a_large_first(api, ctx):
    """more hypotheses than one wait of the host covers, and hypothesis numbers above 2^32: a row is a function of (seed, h) alone"""
    src, tgt, nbr, prm, count = K.HYP_CASES["nr_4_k_5"]
    dsrc, dtgt = _dev(api, ctx, src, 32), _dev(api, ctx, tgt, 16, 1)
    Ts, valid, words = dsrc.initial_alignment_hypotheses(dtgt, nbr, 0, C.ROUND + 40, **prm)
    want = K.hyp_reference("nr_4_k_5")
    _same_hypotheses((Ts[:count], valid[:count], words[:count]), want, "head")
    tail = dsrc.initial_alignment_hypotheses(dtgt, nbr, C.ROUND - 8, 48, **prm)
    _same_hypotheses(tail, (Ts[C.ROUND - 8:], valid[C.ROUND - 8:], words[C.ROUND - 8:]), "across the round")
    from rsreg_amd import api as A
    first = (1 << 40) + 3
    got = dsrc.initial_alignment_hypotheses(dtgt, nbr, first, 8, **prm)
    _same_hypotheses(got, R.hypotheses(A, src, tgt, nbr, prm["seed"], first, 8, prm["nr_samples"], 0.0), "2^40")


# ---- the full call
def _same_result(got, errors, want, label):
    assert got.found == want.found and got.best_hypothesis == want.best_hypothesis, (label, got.best_hypothesis, want.best_hypothesis)
    assert tuple(got.sample) == tuple(want.sample) and tuple(got.match) == tuple(want.match), label
    assert got.n_valid == want.n_valid, (label, got.n_valid, want.n_valid)
    assert got.transform.tobytes() == np.asarray(want.transform, np.float32).tobytes(), label
    assert np.float64(got.error).tobytes() == np.float64(want.error).tobytes(), (label, got.error, want.error)
    assert errors.shape == want.errors.shape and (np.isnan(errors) == np.isnan(want.errors)).all(), label
    ok = ~np.isnan(errors)
    _same_errors(errors[ok], want.errors[ok], label)


@pytest.mark.parametrize("name", K.ALL_ALIGN)
def test_initial_alignment_fields_equal_the_reference(api, ctx, name):
    src, tgt, nbr, guess, prm = K.align_case(name)
    want = K.align_reference(name)
    dsrc, dtgt = _dev(api, ctx, src, 32), _dev(api, ctx, tgt, 16, 1)
    got, errors = dsrc.initial_alignment(dtgt, nbr, guess=guess, errors=True, **prm)
    _same_result(got, errors, want, name)
    again = dsrc.initial_alignment(dtgt, nbr, guess=guess, **prm)                  # (without errors_out)
    assert again.transform.tobytes() == got.transform.tobytes() and again.best_hypothesis == got.best_hypothesis


def test_recovery_of_the_turn(api, ctx):
    """the 120 degrees / 0.5 m motion with 60 % wrong table rows: within 1e-4 Frobenius of the truth"""
    src, tgt, nbr, guess, prm = K.recovery_case()
    got = _dev(api, ctx, src).initial_alignment(_dev(api, ctx, tgt, seed=1), nbr, **prm)
    err = float(np.linalg.norm(got.transform.astype(np.float64) - C.TURN))
    print("recovery: winner %d, %d valid, error %.3g, |T - truth|_F = %.3g" % (got.best_hypothesis, got.n_valid, got.error, err))
    assert got.found and err <= 1e-4


def test_same_bytes_twice_after_other_work_and_from_a_fresh_context(api, ctx):
    src, tgt, nbr, guess, prm = K.ALIGN_CASES["past_a_batch"]
    name = "huber_transforms_%d" % (C.MAX_BATCH + 1)
    s_src, s_tgt, Ts, fn, mcd = K.SCORE_CASES[name]

    def run(c):
        dsrc, dtgt = _dev(api, c, src), _dev(api, c, tgt, seed=1)
        res, errors = dsrc.initial_alignment(dtgt, nbr, errors=True, **prm)
        scores = _dev(api, c, s_src).error_transforms(_dev(api, c, s_tgt, seed=1), Ts, fn, mcd)
        return (res.transform.tobytes(), res.best_hypothesis, res.sample, res.match, res.n_valid, res.error, errors.tobytes(), scores.tobytes())

    first = run(ctx)
    assert run(ctx) == first
    # an unrelated call through the same context, a prerejective call and another, larger pair: every scratch buffer is reused or regrown
    big = _dev(api, ctx, C.box(3000, 77), 48)
    big.normals(10)
    big.error_transforms(_dev(api, ctx, C.box(2000, 78)), C.transforms(40, 1), K.HUBER, 0.09)
    p = C.PREREJ_CASES["k_2"]
    _dev(api, ctx, p[0]).prerejective(_dev(api, ctx, p[1], seed=1), p[2], **p[3])
    assert run(ctx) == first
    fresh = api.Context(0)
    assert run(fresh) == first
    fresh.close()


def test_refusals(api, ctx):
    """the argument checks of the three entry points, which return before anything is launched"""
    from rsreg_amd import lib as L
    src, tgt, nbr, guess, prm = K.ALIGN_CASES["nr_8_k_16"]
    dsrc, dtgt = _dev(api, ctx, src), _dev(api, ctx, tgt, seed=1)
    eye = np.eye(4, dtype=np.float32)
    other = api.Context(0)
    foreign = _dev(api, other, tgt)
    bad_hi, bad_neg, part = nbr.copy(), nbr.copy(), nbr.copy()
    bad_hi[5, 1], bad_neg[9, 0], part[0, 1] = len(tgt), -2, 3                      # (row 0 is a row of -1: now only in part)
    nan = float("nan")
    calls = [lambda: dsrc.error_transforms(dtgt, eye, K.TRUNCATED, 0.0), lambda: dsrc.error_transforms(dtgt, eye, K.TRUNCATED, -1.0),
             lambda: dsrc.error_transforms(dtgt, eye, K.HUBER, nan), lambda: dsrc.error_transforms(dtgt, eye, K.HUBER, 1e-60),
             lambda: dsrc.error_transforms(dtgt, eye, 2, 0.1), lambda: dsrc.error_transforms(dtgt, eye, -1, 0.1),
             lambda: dsrc.error_transforms(foreign, eye, K.TRUNCATED, 0.1)]
    for call in (dsrc.initial_alignment, lambda t, n, **kw: dsrc.initial_alignment_hypotheses(t, n, 0, 4, **kw)):
        calls += [lambda c=call: c(foreign, nbr), lambda c=call: c(dtgt, bad_hi), lambda c=call: c(dtgt, bad_neg), lambda c=call: c(dtgt, part),
                  lambda c=call: c(dtgt, np.zeros((len(src), 17), np.int32)), lambda c=call: c(dtgt, np.zeros((len(src), 0), np.int32)),
                  lambda c=call: c(dtgt, nbr, max_iterations=-1), lambda c=call: c(dtgt, nbr, nr_samples=2), lambda c=call: c(dtgt, nbr, nr_samples=9),
                  lambda c=call: c(dtgt, nbr, error_function=2), lambda c=call: c(dtgt, nbr, error_function=-1),
                  lambda c=call: c(dtgt, nbr, min_sample_distance=-0.1), lambda c=call: c(dtgt, nbr, min_sample_distance=nan),
                  lambda c=call: c(dtgt, nbr, max_correspondence_distance=0.0), lambda c=call: c(dtgt, nbr, max_correspondence_distance=-1.0),
                  lambda c=call: c(dtgt, nbr, max_correspondence_distance=nan), lambda c=call: c(dtgt, nbr, max_correspondence_distance=1e-60)]
    for i, call in enumerate(calls):
        with pytest.raises(L.RsregError) as e:
            call()
        assert e.value.status == L.RSREG_ERR_INVALID_ARG, i
    foreign.close()
    other.close()
    # and what is no error: no transform, +inf as thr, a min_sample_distance whose square is +inf
    assert len(dsrc.error_transforms(dtgt, np.zeros((0, 4, 4), np.float32), K.TRUNCATED, 0.1)) == 0
    assert dsrc.error_transforms(dtgt, eye, K.TRUNCATED, math.inf)[0] == 0.0
    res = dsrc.initial_alignment(dtgt, nbr, min_sample_distance=1e200, max_iterations=4)
    assert not res.found and res.n_valid == 0 and res.error == math.inf


def test_python_class(api, ctx):
    """api.SampleConsensusInitialAlignment: feature_knn, then initial_alignment, then the source moved by the result -- from device
    clouds and from host clouds"""
    src, tgt, true_of = C.pair(120, 3)
    rng = np.random.default_rng(2)
    fsrc = rng.random((len(src), 33)).astype(np.float32)            # descriptors that tell the records apart
    ftgt = np.empty_like(fsrc)
    ftgt[true_of] = fsrc
    as_rec = lambda f: np.ascontiguousarray(f).view(api.FPFH_DTYPE).reshape(-1)
    hfs, hft = (api.FPFHCloud(as_rec(f), len(f), 1, True) for f in (fsrc, ftgt))
    hsrc, htgt = (api.NormalCloud(S.records(x, 32, s), len(x), 1, False) for x, s in ((src, 0), (tgt, 1)))
    dfs, dft = api.DeviceCloud(hfs, ctx=ctx), api.DeviceCloud(hft, ctx=ctx)
    dsrc, dtgt = api.DeviceCloud(hsrc, ctx=ctx), api.DeviceCloud(htgt, ctx=ctx)
    prm = dict(max_iterations=64, max_correspondence_distance=K.THR, min_sample_distance=0.3, nr_samples=4, error_function=K.HUBER, seed=5)
    nbr, _ = dfs.feature_knn(dft, 3)
    assert (nbr[:, 0] == true_of).all()
    res = dsrc.initial_alignment(dtgt, nbr, **prm)
    want = R.initial_alignment(api, src, tgt, nbr, **prm)
    assert res.found and res.best_hypothesis == want.best_hypothesis and res.transform.tobytes() == np.asarray(want.transform, np.float32).tobytes()
    moved = api.transformPointCloud(dsrc, res.transform)
    n, stride = moved.info()[:2]
    from rsreg_amd import lib as L
    b = np.zeros(n * stride, np.uint8)
    L.check(L.lib().rsreg_cloud_download(moved.h, b.ctypes.data, n), ctx.h)
    for clouds in ((dsrc, dtgt, dfs, dft), (hsrc, htgt, hfs, hft)):
        reg = api.SampleConsensusInitialAlignment(ctx)
        reg.setInputSource(clouds[0])
        reg.setInputTarget(clouds[1])
        reg.setSourceFeatures(clouds[2])
        reg.setTargetFeatures(clouds[3])
        reg.setMaximumIterations(64)
        reg.setNumberOfSamples(4)
        reg.setCorrespondenceRandomness(3)
        reg.setMinSampleDistance(0.3)
        reg.setMaxCorrespondenceDistance(K.THR)
        reg.setErrorFunction(api.SCIA_HUBER)
        reg.setSeed(5)
        assert reg.getMinSampleDistance() == 0.3 and reg.getNumberOfSamples() == 4 and reg.getCorrespondenceRandomness() == 3
        out = reg.align()
        assert reg.hasConverged() and reg.getFinalTransformation().tobytes() == res.transform.tobytes() and reg.getFitnessScore() == res.error
        if isinstance(clouds[0], api.DeviceCloud):
            a = np.zeros(n * stride, np.uint8)
            L.check(L.lib().rsreg_cloud_download(out.h, a.ctypes.data, n), ctx.h)
        else:
            a = np.ascontiguousarray(out.points).view(np.uint8).reshape(-1)
        xyz = lambda raw: raw.view(np.float32).reshape(n, stride // 4)[:, :3]
        assert xyz(a).tobytes() == xyz(b).tobytes()
        assert np.abs(xyz(a) - tgt[true_of]).max() < 1e-5
    # a guess that is already the answer keeps its bytes: nothing beats an error of rounding
    reg.setMaximumIterations(8)
    reg.align(guess=res.transform)
    assert reg.getFinalTransformation().tobytes() == res.transform.tobytes() or reg.hasConverged()
