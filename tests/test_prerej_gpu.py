"""rsreg_cloud_score_transforms and rsreg_cloud_prerejective (pcl::SampleConsensusPrerejective: poses from descriptor neighbours,
scored against the whole target cloud by an exact nearest-point search) on the GPU and the Python adaptor, against
tests/prerej_ref.py on the cases of tests/prerej_cases.py.

Counts, sums, the number of valid hypotheses, the winner, its sample and matches, all 16 floats of the transform, the fitness and the
inlier list are EQUAL to the reference: the contract (include/rsreg.h) fixes the generator, the operation order of a score, the
order of the sum and the selection, so there is no tolerance.
"""
import functools

import numpy as np
import pytest

import prerej_cases as C
import prerej_ref as R
import sac_cases as K

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
    return api.DeviceCloud(api.NormalCloud(K.records(xyz, stride, seed), len(xyz), 1, False), ctx=ctx)


@functools.lru_cache(maxsize=None)
def _score_reference(name):
    src, tgt, Ts, rng = C.SCORE_CASES[name]
    return R.score_transforms(Ts, src, tgt, rng)


@functools.lru_cache(maxsize=None)
def _prerej_reference(name):
    from rsreg_amd import api
    src, tgt, nbr, prm = C.PREREJ_CASES[name] if name != "end_to_end" else C.end_to_end()
    return R.prerejective(api, src, tgt, nbr, **prm)


def _same_scores(got, want, label):
    counts, sums = got
    assert counts.dtype == np.uint32 and sums.dtype == np.float64 and counts.shape == sums.shape == want[0].shape
    bad = np.flatnonzero(counts != want[0])
    assert len(bad) == 0, (label, bad[:5], counts[bad[:5]], want[0][bad[:5]])
    bad = np.flatnonzero(sums.view(np.uint64) != want[1].view(np.uint64))
    assert len(bad) == 0, (label, bad[:5], sums[bad[:5]], want[1][bad[:5]])


@pytest.mark.parametrize("name", list(C.SCORE_CASES))
def test_score_transforms_equals_the_reference(api, ctx, name):
    src, tgt, Ts, rng = C.SCORE_CASES[name]
    _same_scores(_dev(api, ctx, src).score_transforms(_dev(api, ctx, tgt, seed=1), Ts, rng), _score_reference(name), name)


def test_score_transforms_record_layouts_and_one_cloud(api, ctx):
    src, tgt, Ts, rng = C.SCORE_CASES["source_129"]
    want = _score_reference("source_129")
    for ss, ts in zip(C.STRIDES, reversed(C.STRIDES)):
        _same_scores(_dev(api, ctx, src, ss).score_transforms(_dev(api, ctx, tgt, ts, 1), Ts, rng), want, (ss, ts))
    # source == target: under the identity every finite record finds itself at d2 = 0
    one = _dev(api, ctx, tgt, 32)
    got = one.score_transforms(one, Ts, rng)
    _same_scores(got, R.score_transforms(Ts, tgt, tgt, rng), "one cloud")
    assert got[0][0] == len(tgt) and got[1][0] == 0.0


def test_score_transforms_one_call_equals_one_call_each(api, ctx):
    src, tgt, Ts, rng = C.SCORE_CASES["hypotheses_past_a_batch"]
    dsrc, dtgt = _dev(api, ctx, src), _dev(api, ctx, tgt, seed=1)
    counts, sums = dsrc.score_transforms(dtgt, Ts, rng)
    for h in list(range(14)) + [C.MAX_BATCH - 1, C.MAX_BATCH]:
        c1, s1 = dsrc.score_transforms(dtgt, Ts[h], rng)
        assert c1[0] == counts[h] and s1.view(np.uint64)[0] == sums.view(np.uint64)[h], h


def _same_result(got_inliers, got, want, label=""):
    assert got.found == want.found and got.best_hypothesis == want.best_hypothesis, (label, got.best_hypothesis, want.best_hypothesis)
    assert tuple(got.sample) == tuple(want.sample) and tuple(got.match) == tuple(want.match), label
    assert got.n_valid == want.n_valid and got.n_inliers == want.n_inliers and got.n_out == len(want.inliers), (label, got.n_valid, want.n_valid)
    assert got.transform.tobytes() == np.asarray(want.transform, np.float32).tobytes(), label
    assert np.float64(got.fitness).tobytes() == np.float64(want.fitness).tobytes(), (label, got.fitness, want.fitness)
    assert got_inliers.dtype == np.int32 and got_inliers.tobytes() == want.inliers.tobytes(), label


@pytest.mark.parametrize("name", list(C.PREREJ_CASES))
def test_prerejective_fields_equal_the_reference(api, ctx, name):
    src, tgt, nbr, prm = C.PREREJ_CASES[name]
    want = _prerej_reference(name)
    dsrc, dtgt = _dev(api, ctx, src, 32), _dev(api, ctx, tgt, 16, 1)
    inliers, got = dsrc.prerejective(dtgt, nbr, **prm)
    _same_result(inliers, got, want, name)
    # the per-hypothesis counts and sums of the valid hypotheses, through the scoring stage on its own
    valid = np.flatnonzero(want.valid)[:40]
    if len(valid):
        Ts = np.array([R.hypothesis(api, R.xyz_of(src), R.xyz_of(tgt), nbr, prm.get("seed", 0), int(h), prm.get("similarity_threshold", 0.9))[0] for h in valid])
        rng = prm.get("max_correspondence_distance", float(np.sqrt(np.finfo(np.float64).max)))
        _same_scores(dsrc.score_transforms(dtgt, Ts, rng), (want.counts[valid], want.sums[valid]), name)
    if not want.found:
        assert (got.transform == np.eye(4)).all() and got.n_inliers == 0 and got.fitness == 0.0 and len(inliers) == 0
        return
    # every capacity around n_inliers: the first `capacity` records, the full number reported
    for room in sorted({0, 1, want.n_inliers - 1, want.n_inliers, want.n_inliers + 1}):
        few, again = dsrc.prerejective(dtgt, nbr, capacity=room, **prm)
        assert again.n_out == want.n_inliers and len(few) == min(room, want.n_inliers) and few.tobytes() == want.inliers[:room].tobytes(), (name, room)
        assert again.transform.tobytes() == got.transform.tobytes()


def test_prerejective_at_the_fraction_bound(api, ctx):
    """inlier_fraction exactly count / ns of the best-supported hypothesis: AT the bound it qualifies, one step above nothing does"""
    src, tgt, nbr, prm = C.PREREJ_CASES["fraction_0"]
    top = _prerej_reference("fraction_half")
    best = int(top.counts.max())
    frac = float(best) / float(len(src))
    dsrc, dtgt = _dev(api, ctx, src), _dev(api, ctx, tgt, seed=1)
    for f, found in ((frac, True), (float(np.nextafter(frac, 2.0)), False)):
        p = dict(prm, inlier_fraction=f)
        want = R.prerejective(api, src, tgt, nbr, **p)
        inliers, got = dsrc.prerejective(dtgt, nbr, **p)
        _same_result(inliers, got, want, f)
        assert got.found == found and (not found or got.n_inliers == best)


def test_same_bytes_twice_after_other_work_and_from_a_fresh_context(api, ctx):
    src, tgt, nbr, prm = C.PREREJ_CASES["past_a_batch"]
    s_src, s_tgt, Ts, rng = C.SCORE_CASES["hypotheses_past_a_batch"]

    def run(c):
        dsrc, dtgt = _dev(api, c, src), _dev(api, c, tgt, seed=1)
        inliers, res = dsrc.prerejective(dtgt, nbr, **prm)
        counts, sums = _dev(api, c, s_src).score_transforms(_dev(api, c, s_tgt, seed=1), Ts, rng)
        return (inliers.tobytes(), res.transform.tobytes(), res.best_hypothesis, res.sample, res.match, res.n_valid, res.n_inliers, res.fitness,
                counts.tobytes(), sums.tobytes())

    first = run(ctx)
    assert run(ctx) == first
    # an unrelated call through the same context, and another, larger pair of clouds: every scratch buffer is reused or regrown
    big = _dev(api, ctx, C.box(3000, 77), 48)
    big.normals(10)
    big.score_transforms(_dev(api, ctx, C.box(2000, 78)), C.transforms(40, 1), 0.3)
    assert run(ctx) == first
    fresh = api.Context(0)
    assert run(fresh) == first
    fresh.close()


def test_refusals(api, ctx):
    """the argument checks of both entry points, which return before anything is launched (they need a context, hence a device)"""
    from rsreg_amd import lib as L
    src, tgt, nbr, prm = C.PREREJ_CASES["k_2"]
    dsrc, dtgt = _dev(api, ctx, src), _dev(api, ctx, tgt, seed=1)
    eye = np.eye(4, dtype=np.float32)
    other = api.Context(0)
    foreign = _dev(api, other, tgt)
    bad_hi, bad_neg, part = nbr.copy(), nbr.copy(), nbr.copy()
    bad_hi[5, 1], bad_neg[9, 0], part[0, 1] = len(tgt), -2, 3                      # (row 0 is a row of -1: now only in part)
    calls = [lambda: dsrc.score_transforms(dtgt, eye, -1.0), lambda: dsrc.score_transforms(dtgt, eye, float("nan")),
             lambda: dsrc.score_transforms(foreign, eye, 0.1), lambda: dsrc.prerejective(foreign, nbr, **prm),
             lambda: dsrc.prerejective(dtgt, bad_hi, **prm), lambda: dsrc.prerejective(dtgt, bad_neg, **prm), lambda: dsrc.prerejective(dtgt, part, **prm),
             lambda: dsrc.prerejective(dtgt, np.zeros((len(src), 17), np.int32), **prm), lambda: dsrc.prerejective(dtgt, np.zeros((len(src), 0), np.int32), **prm),
             lambda: dsrc.prerejective(dtgt, nbr, max_iterations=-1), lambda: dsrc.prerejective(dtgt, nbr, similarity_threshold=1.0),
             lambda: dsrc.prerejective(dtgt, nbr, similarity_threshold=-0.1), lambda: dsrc.prerejective(dtgt, nbr, similarity_threshold=float("nan")),
             lambda: dsrc.prerejective(dtgt, nbr, inlier_fraction=1.5), lambda: dsrc.prerejective(dtgt, nbr, inlier_fraction=-0.1),
             lambda: dsrc.prerejective(dtgt, nbr, max_correspondence_distance=-1.0), lambda: dsrc.prerejective(dtgt, nbr, max_correspondence_distance=float("nan"))]
    for i, call in enumerate(calls):
        with pytest.raises(L.RsregError) as e:
            call()
        assert e.value.status == L.RSREG_ERR_INVALID_ARG, i
    foreign.close()
    other.close()
    # and what is no error: no transform, an empty source, an empty target
    counts, sums = dsrc.score_transforms(dtgt, np.zeros((0, 4, 4), np.float32), 0.1)
    assert len(counts) == 0 and len(sums) == 0
    empty = _dev(api, ctx, np.zeros((0, 3), np.float32))
    assert (dsrc.score_transforms(empty, eye, 0.1)[0] == 0).all() and (empty.score_transforms(dtgt, eye, 0.1)[0] == 0).all()
    inliers, res = dsrc.prerejective(empty, np.full((len(src), 2), -1, np.int32), **prm)
    assert not res.found and len(inliers) == 0 and res.n_valid == 0


def test_end_to_end_on_a_constructed_pair(api, ctx):
    """400 points in the unit box and their copy moved by 120 degrees and 0.5 m; 40 % of the rows of the neighbour table hold the
    true match among k = 5, the rest are random; range 0.05, 512 iterations, select_by_inliers.  The reference (on the CPU:
    tests/test_prerej_cpu.py) finds every source record an inlier with this seed, winner 195, |T - truth|_F = 1.04e-07; the bar
    on the GPU's pose is twice that, 2.08e-07 -- and the transform is bit-equal to the reference's anyway."""
    src, tgt, nbr, prm = C.end_to_end()
    want = _prerej_reference("end_to_end")
    inliers, got = _dev(api, ctx, src).prerejective(_dev(api, ctx, tgt, seed=1), nbr, **prm)
    err = float(np.linalg.norm(got.transform.astype(np.float64) - C.TURN))
    ref_err = float(np.linalg.norm(np.asarray(want.transform, np.float64) - C.TURN))
    print("end to end: winner %d, %d valid, %d inliers, |T - truth|_F = %.3g (reference %.3g)" % (got.best_hypothesis, got.n_valid, got.n_inliers, err, ref_err))
    assert got.found and got.n_inliers == len(src) and (inliers == np.arange(len(src))).all()
    _same_result(inliers, got, want, "end to end")
    assert err <= 2 * 1.04e-07


def test_python_class(api, ctx):
    """api.SampleConsensusPrerejective: feature_knn, then prerejective, then the source moved by the result"""
    src, tgt, true_of = C.pair(120, 3)
    rng = np.random.default_rng(2)
    # descriptors that tell the records apart: the target's rows are its source record's rows
    fsrc = rng.random((len(src), 33)).astype(np.float32)
    ftgt = np.empty_like(fsrc)
    ftgt[true_of] = fsrc
    as_rec = lambda f: np.ascontiguousarray(f).view(api.FPFH_DTYPE).reshape(-1)
    dfs, dft = (api.DeviceCloud(api.FPFHCloud(as_rec(f), len(f), 1, True), ctx=ctx) for f in (fsrc, ftgt))
    dsrc, dtgt = _dev(api, ctx, src, 32), _dev(api, ctx, tgt, 32, 1)
    reg = api.SampleConsensusPrerejective(ctx)
    reg.setInputSource(dsrc)
    reg.setInputTarget(dtgt)
    reg.setSourceFeatures(dfs)
    reg.setTargetFeatures(dft)
    reg.setMaximumIterations(64)
    reg.setNumberOfSamples(3)
    reg.setCorrespondenceRandomness(3)
    reg.setSimilarityThreshold(0.9)
    reg.setMaxCorrespondenceDistance(C.RANGE)
    reg.setInlierFraction(0.25)
    with pytest.raises(Exception):
        reg.setNumberOfSamples(4)
    out = reg.align()
    nbr, _ = dfs.feature_knn(dft, 3)
    assert (nbr[:, 0] == true_of).all()
    inliers, res = dsrc.prerejective(dtgt, nbr, max_iterations=64, similarity_threshold=0.9, max_correspondence_distance=C.RANGE, inlier_fraction=0.25)
    want = R.prerejective(api, src, tgt, nbr, max_iterations=64, similarity_threshold=0.9, max_correspondence_distance=C.RANGE, inlier_fraction=0.25)
    _same_result(inliers, res, want, "class")
    assert reg.hasConverged() and reg.getFinalTransformation().tobytes() == res.transform.tobytes()
    assert (reg.getInliers() == inliers).all() and reg.getFitnessScore() == res.fitness
    moved = api.transformPointCloud(dsrc, res.transform)
    n, stride, w, h, dense = out.info()
    assert n == len(src) and stride == 32
    a, b = np.zeros(n * stride, np.uint8), np.zeros(n * stride, np.uint8)
    from rsreg_amd import lib as L
    L.check(L.lib().rsreg_cloud_download(out.h, a.ctypes.data, n), ctx.h)
    L.check(L.lib().rsreg_cloud_download(moved.h, b.ctypes.data, n), ctx.h)
    assert a.tobytes() == b.tobytes()
    xyz = a.view(np.float32).reshape(n, 8)[:, :3]
    assert np.abs(xyz - tgt[true_of]).max() < 1e-5
