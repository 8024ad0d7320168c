"""What every case of tests/sac_edge_cases.py is FOR, asserted on the reference (tests/sac_ref.py) without a GPU, so that
tests/test_sac_edges_gpu.py compares bits on cases that are proven to reach the branch they name: degenerate three-pair samples, the
edges of the stopping rule, the large list's plan, and -- from the reference's own float32 intermediates (sac_ref.Trace) -- in which
regime of the float32 range each scaled cloud lies.  (sac_ref.replay asserts its k-margin for every case run here.)
"""
import math

import numpy as np
import pytest

import sac_cases as K
import sac_edge_cases as E
import sac_ref as R


@pytest.fixture(scope="module")
def api(rs):
    from rsreg_amd import api
    return api


def _sample_sigma(P, Q, ids):
    """the singular values of the three pairs' cross-covariance, float64 (numpy: an estimate of the rank the solve will see)"""
    p, q = P[list(ids)].astype(np.float64), Q[list(ids)].astype(np.float64)
    return np.linalg.svd((q - q.mean(axis=0)).T @ (p - p.mean(axis=0)) / 3.0, compute_uv=False)


def _collinear(P, ids):
    a, b, c = (P[i].astype(np.float64) for i in ids)
    return (np.cross(b - a, c - a) == 0).all() and np.linalg.norm(b - a) > 0 and np.linalg.norm(c - a) > 0


def test_degenerate_samples(api):
    for name in ("collinear", "collinear_exact_turn"):
        r, src, tgt, corr, true, prm = E.reference(name)
        P, Q, finite = R.pair_points(src, tgt, corr)
        assert r.valid[:r.iterations].all() and r.valid.all() and r.found and r.n_inliers == len(corr) == 300 and r.iterations == 1
        assert _collinear(P, r.sample)                                  # the cross product in float64 is exactly 0
        s = _sample_sigma(P, Q, r.sample)
        print(name, "singular values of the winner's cross-covariance:", s)
        # collinear sources: the cross-covariance is (a vector) x (the line's direction)^T, rank 1 whatever the targets are.  By the
        # solve's rule (s > 1e-13 * s_max) complete_u3 fills TWO columns of U
        assert s[1] < 1e-13 * s[0] and s[2] < 1e-13 * s[0]
        assert np.abs(np.linalg.det(r.transform[:3, :3].astype(np.float64)) - 1) < 1e-5
    r, src, tgt, corr, true, prm = E.reference("collinear_noisy")
    P, Q, finite = R.pair_points(src, tgt, corr)
    assert r.found and r.valid.all() and 1 < r.best_hypothesis + 1 < r.iterations < prm["max_iterations"]      # several hypotheses are consumed
    assert r.n_inliers == true.sum() == 180 and (r.flags == true).all() and _collinear(P, r.sample) and true[list(r.sample)].all()
    assert set(r.counts[:r.iterations].tolist()) == {0, 180}             # a sample with a random target fits no pair at all

    r, src, tgt, corr, true, prm = E.reference("one_target")
    P, Q, finite = R.pair_points(src, tgt, corr)
    assert (Q == Q[0]).all() and _collinear(P, r.sample)
    assert r.valid.all() and r.found and 3 <= r.n_inliers < 20 and r.iterations == prm["max_iterations"]
    assert (_sample_sigma(P, Q, r.sample) < 1e-13).all()                 # no target differs: rank 0 up to rounding

    r, src, tgt, corr, true, prm = E.reference("coplanar_mirrored")
    P, Q, finite = R.pair_points(src, tgt, corr)
    assert (Q == P * np.float32([1, 1, -1])).all() and r.valid.all() and r.found and 3 <= r.n_inliers < 30
    T = r.transform.astype(np.float64)
    # the answer is a TURN that takes the sample's triangle onto its mirror image, not the mirror
    assert abs(np.linalg.det(T[:3, :3]) - 1) < 1e-5 and np.abs(T[:3, :3] - np.diag([1, 1, -1])).max() > 0.1
    ids = list(r.sample)
    assert np.abs(P[ids].astype(np.float64) @ T[:3, :3].T + T[:3, 3] - Q[ids]).max() < 1e-5
    s = _sample_sigma(P, Q, r.sample)
    assert s[2] < 1e-13 * s[0] < s[1]                                    # rank 2: the third column of U is completed, its sign by the determinant rule
    assert not r.flags.all() and r.flags[ids].all()

    for name, denormal in (("coincident_sources_apart_by_one_ulp", False), ("coincident_sources_apart_by_one_ulp_denormal_d2", True)):
        r, src, tgt, corr, true, prm = E.reference(name)
        P, Q, finite = R.pair_points(src, tgt, corr)
        assert r.valid.all() and r.found and r.iterations == 1 and r.n_inliers == 300 and prm.get("min_sample_distance", 0.0) == 0.0
        i = list(r.sample)
        d2 = [float(R.l2_simple(P[i[a]], P[i[b]])) for a, b in ((0, 1), (0, 2), (1, 2))]
        ulp = np.spacing(P[:, 0]).max()
        assert (np.abs(P[:, 0] - P[0, 0]) <= 300 * ulp).all() and (P[:, 1:] == P[0, 1:]).all()         # within 300 last-bit steps of x, y and z equal
        if denormal:
            assert all(0 < d < float(E.FLT_MIN) for d in d2), d2         # positive denormals: d2 > 0 holds only if they are kept
            assert (Q == Q[0]).all()
        else:
            assert all(float(E.FLT_MIN) < d < 1e-9 for d in d2), d2


def test_rule_edges(api):
    r, src, tgt, corr, true, prm = E.reference("all_inliers")
    assert true.all() and r.found and r.n_inliers == len(corr) and r.iterations == 1 and r.best_hypothesis == 0
    assert r.ks == [math.log(1 - 0.99) / math.log(R.EPS)] and 0.127 < r.ks[0] < 0.128          # q clamped to DBL_EPSILON

    r, src, tgt, corr, true, prm = E.reference("n3")
    first_invalid = int(np.flatnonzero(~r.valid)[0])
    assert len(corr) == 3 and r.valid[0] and 0 < (~r.valid).sum() < 50 and r.found and r.n_inliers == 3 and r.iterations == 1
    assert sorted(r.sample) == [0, 1, 2]
    r0 = E.reference("n3_threshold_zero")[0]
    assert (r0.valid == r.valid).all() and not r0.found and r0.iterations == 50 > first_invalid and r0.best == 0     # an invalid hypothesis is passed over
    for name, n in (("n4", 4), ("n5", 5)):
        r, src, tgt, corr, true, prm = E.reference(name)
        assert len(corr) == n and r.found and r.n_inliers == n and r.iterations == 1

    r, src, tgt, corr, true, prm = E.reference("threshold_zero")
    assert prm["inlier_threshold"] == 0.0 and not r.found and r.valid.all() and r.iterations == prm["max_iterations"] == 100
    assert r.best == 0 and (r.counts == 0).all() and len(r.ks) == 1 and 2.07e16 < r.ks[0] < 2.08e16 and len(r.kept) == len(corr)

    r = E.reference("max_iterations_0")[0]
    assert not r.found and r.iterations == 0 and r.best == -1
    r, src, tgt, corr, true, prm = E.reference("max_iterations_1")
    assert r.found and r.iterations == 1 and r.best_hypothesis == 0 and 3 <= r.n_inliers < len(corr) and r.ks[0] > 1

    r, src, tgt, corr, true, prm = E.reference("probability_1e-300")
    assert math.log(1.0 - 1e-300) == 0.0 and r.ks == [0.0] and math.copysign(1.0, r.ks[0]) == -1.0                   # k = 0 / log(q) = -0.0
    assert r.valid[0] and r.iterations == 1 and r.best == 0 and not r.found                                          # NO MODEL although hypothesis 0 is valid
    r, src, tgt, corr, true, prm = E.reference("probability_1e-300_found")
    assert r.ks == [0.0] and math.copysign(1.0, r.ks[0]) == -1.0 and r.iterations == 1 and r.found and r.n_inliers == true.sum()

    # the largest double below 1 is 1 - 2^-53 = 0.9999999999999999 and runs; 1 - 2^-54 is not a double: it rounds to 1.0, which is refused
    r, src, tgt, corr, true, prm = E.reference("probability_0.9999999999999999")
    assert prm["probability"] == 1.0 - 2.0 ** -53 == np.nextafter(1.0, 0.0) and 1.0 - 2.0 ** -54 == 1.0
    assert r.found and r.n_inliers == len(corr) and abs(r.ks[0] - 53.0 / 52.0) < 1e-12 and len(r.ks) == 1 and r.iterations == 2                      # log(2^-53) / log(2^-52): ONE hypothesis more

    r, src, tgt, corr, true, prm = E.reference("deep")
    batches, done = [], 0
    while K.batch(done, prm["max_iterations"]):
        batches.append(K.batch(done, prm["max_iterations"]))
        done += batches[-1]
    assert batches == [256, 512, 1024, 2048, 4096, 1064] and r.iterations == 9000 == prm["max_iterations"] and r.found
    assert r.ks[-1] > 9000 and r.best_hypothesis >= K.FIRST_BATCH and r.n_inliers >= true.sum() == 150

    for name, seed in (("seed_2^63", 1 << 63), ("seed_2^64-3", (1 << 64) - 3)):
        r, src, tgt, corr, true, prm = E.reference(name)
        assert prm["seed"] == seed >= 1 << 63 and r.found and r.best_hypothesis > 0 and r.iterations < prm["max_iterations"]
    assert E.reference("seed_2^63")[0].sample != E.reference("seed_2^64-3")[0].sample


def test_large_list(api):
    r, src, tgt, corr, true, prm = E.reference("big")
    assert len(corr) == E.BIG_N and r.found and max(r.sample) > 65535 and r.n_inliers >= true.sum() == 35000 and r.n_inliers < len(corr)
    assert K.plan(E.BIG_N, E.BIG_H) == (137, 64, 3, 22) and 64 % 3 != 0              # 137 pair tiles, slices of three chunks, the last one ragged
    assert -(-E.BIG_N // 1024) == 69                                                 # scan tiles
    tiles, chunks, per, slices = K.plan(E.EXACT_N, E.BIG_H)
    assert tiles * chunks == K.MAX_GROUPS and per == 1 and E.EXACT_N < E.BIG_N
    assert K.plan(E.EXACT_N + 1, E.BIG_H)[2] == 2
    base, pick = E.transforms_fast_pick(E.BIG_H)
    assert (K.transforms_fast(E.BIG_H) == base[pick]).all() and len(base) == 331


def _trace(api, name):
    """(Trace over the sample checks and the scores of every hypothesis the replay consumed, the sample d2 seen, the winner's d2)"""
    r, src, tgt, corr, true, prm = E.reference(name)
    P, Q, finite = R.pair_points(src, tgt, corr)
    tr, sample_d2 = R.Trace(), []
    for h in range(r.iterations):
        T, ids, good = R.hypothesis(api, P, Q, finite, prm["seed"], h)
        for t in range(R.TRIES if good < 0 else good + 1):
            i = [int(R.draw_index(prm["seed"], h, 3 * t + k, len(P))) for k in range(3)]
            if len(set(i)) == 3:
                sample_d2 += [float(tr.l2_simple(P[i[a]], P[i[b]])) for a, b in ((0, 1), (0, 2), (1, 2))]
        if T is not None:
            d2 = tr.score(T, P, Q)
            assert (((d2.astype(np.float64) < prm["inlier_threshold"] * prm["inlier_threshold"]) & finite) == R.within(T, P, Q, finite, prm["inlier_threshold"])).all()
    winner_d2 = R.Trace().score(r.transform, P, Q) if r.found else None
    return r, tr, np.array(sample_d2), winner_d2


def test_float32_range_regimes(api):
    """Each scaled cloud classified from the reference's own float32 intermediates.  IN THE WINDOW (no operation overflows, gives a
    non-zero denormal or underflows to 0) scaling by 2^e commutes with every operation of the contract, so the result must be the
    scale-1 result: counts, samples, iterations and kept equal, the rotation's bits equal, the translation times 2^e."""
    one, tr1, s1, w1 = _trace(api, "scale_1")
    assert (tr1.inf, tr1.nan, tr1.denormal, tr1.underflow) == (0, 0, 0, 0) and one.found and one.best_hypothesis > 0
    regimes = {}
    for e in E.SCALE_EXPONENTS:
        r, tr, sample_d2, winner_d2 = _trace(api, "scale_2^%+d" % e)
        kinds = [k for k in ("inf", "nan", "denormal", "underflow") if getattr(tr, k)]
        regimes[e] = "in-window" if not kinds else "+".join(kinds)
        print("2^%+d: %s (inf %d, nan %d, denormal %d, underflow %d); found %d, %d inliers, iterations %d, valid %d" %
              (e, regimes[e], tr.inf, tr.nan, tr.denormal, tr.underflow, r.found, r.n_inliers, r.iterations, r.valid.sum()))
        if not kinds:
            assert (r.counts == one.counts).all() and (r.valid == one.valid).all()
            assert (r.found, r.best_hypothesis, r.sample, r.iterations, r.n_inliers) == (one.found, one.best_hypothesis, one.sample, one.iterations, one.n_inliers)
            assert r.kept.tobytes() == one.kept.tobytes()
            assert r.transform[:3, :3].tobytes() == one.transform[:3, :3].tobytes()
            assert r.transform[:3, 3].tobytes() == np.ldexp(one.transform[:3, 3], e).astype(np.float32).tobytes()
        if e == -100:         # every squared distance between two source points underflows to 0: "coincident", no valid sample
            assert len(sample_d2) > 0 and (sample_d2 == 0).all() and tr.underflow > 0 and not r.valid.any() and not r.found and r.iterations == 1
        if e == 100:          # threshold^2 is above FLT_MAX: exactly the pairs with a finite d2 count
            assert E.scale_prm(e)["inlier_threshold"] * E.scale_prm(e)["inlier_threshold"] > float(E.FLT_MAX) and tr.inf > 0 and r.found
            assert r.n_inliers == np.isfinite(winner_d2).sum() < len(r.flags) and np.isinf(winner_d2).any()
    assert regimes[-30] == regimes[30] == "in-window"
    assert all("inf" in regimes[e] for e in (62, 70, 100)) and all(regimes[e] != "in-window" and "inf" not in regimes[e] for e in (-62, -70, -100))
    assert "denormal" in regimes[-62] and "underflow" in regimes[-70]

    r, tr, sample_d2, _ = _trace(api, "denormal_cloud")
    assert len(sample_d2) > 0 and (sample_d2 == 0).all() and not r.valid.any() and not r.found and r.iterations == 1


def test_range_thresholds(api):
    t_inf, t_big, t_tiny, t_zero = E.RANGE_THRESHOLDS
    assert t_inf * t_inf == math.inf and float(E.FLT_MAX) < t_big * t_big < math.inf and 0 < t_tiny * t_tiny < 2.0 ** -149 and t_zero * t_zero == 0.0
    src, tgt, corr, d2 = E.range_threshold_pairs()
    assert d2[0] == d2[1] == 0 and d2[2] == 2.0 ** -149 and d2[3] == 2.0 ** -148 and d2[4] == 2.0 ** -147 and d2[5] == 0.0625
    assert np.isfinite(d2[:9]).all() and d2[8] > 3.38e38 and np.isinf(d2[9:12]).all() and np.isnan(d2[12])
    P, Q, finite = R.pair_points(src, tgt, corr)
    eye = np.eye(4, dtype=np.float32)[None]
    assert [int(R.count_inliers(eye, P, Q, finite, t)[0]) for t in E.RANGE_THRESHOLDS] == [9, 9, 2, 0]
    # the rejector at these thresholds
    n = 400
    for name in ("threshold_1e200", "threshold_2e19"):
        r = E.reference(name)[0]
        assert r.found and r.n_inliers == n and r.iterations == 1
    r, src, tgt, corr, true, prm = E.reference("threshold_1e-30")
    P, Q, finite = R.pair_points(src, tgt, corr)
    assert r.found and 3 <= r.n_inliers < 100 and r.n_inliers == (R.Trace().score(r.transform, P, Q) == 0).sum()      # d2 < 2^-149 is d2 == 0
    r = E.reference("threshold_1e-200")[0]
    assert not r.found and r.best == 0 and r.iterations == E.SCALE_IT
    # thresholds whose square IS a float: a pair with d2 == threshold^2 is outside
    for thr in (0.5, 2.0 ** -10):
        src, tgt, corr, d2 = K.threshold_pairs(thr)
        f = np.float32(thr * thr)
        assert float(f) == thr * thr and (d2[8:16] == f).all() and (d2[:8] < f).all() and (d2[16:] > f).all()
        P, Q, finite = R.pair_points(src, tgt, corr)
        got = R.within(np.eye(4, dtype=np.float32), P, Q, finite, thr)
        assert got[:8].all() and not got[8:].any()


def test_extreme_transforms(api):
    src, tgt, corr, Ts = E.extreme_transforms_case()
    P, Q, finite = R.pair_points(src, tgt, corr)
    assert finite.all()
    counts = R.count_inliers(Ts, P, Q, finite, E.RANGE_THRESHOLDS[0])
    nan_rows = inf_rows = 0
    for T, c in zip(Ts, counts):
        tr = R.Trace()
        d2 = tr.score(T, P, Q)
        # threshold^2 = +inf: a pair counts iff its d2 is finite; NaN (inf - inf on the way) and +inf never do
        assert c == np.isfinite(d2).sum() and not (np.isfinite(d2) & ~np.isfinite(Trace_moved_max(T, P))).any()
        nan_rows += np.isnan(d2).any()
        inf_rows += np.isinf(d2).any()
    print("extreme transforms: counts", counts.tolist())
    assert nan_rows >= 4 and inf_rows >= 10 and (counts > 0).sum() >= 10 and len(set(counts.tolist())) >= 8
    assert (Ts[[1, 9, 11, 12]] == 0).any() and np.signbit(Ts[[1, 9, 11, 12]]).any()                                  # -0.0 is there
    assert (np.abs(Ts[np.nonzero(Ts)]) < E.FLT_MIN).any() and (np.abs(Ts) == E.FLT_MAX).any()


def Trace_moved_max(T, P):
    """per pair: the largest magnitude among the three coordinates of the moved point (NaN if any is NaN): a d2 can be finite only
    if the moved point is -- an intermediate +inf never comes back"""
    m = np.asarray(T, np.float32)
    tr = R.Trace()
    out = []
    for r in range(3):
        a = tr.add(tr.mul(m[r, 0], P[:, 0]), tr.mul(m[r, 1], P[:, 1]))
        out.append(tr.add(tr.add(a, tr.mul(m[r, 2], P[:, 2])), m[r, 3]))
    with np.errstate(all="ignore"):
        return np.abs(np.stack(out)).max(axis=0)


def test_few_finite_pairs():
    for k in (2, 3):
        src, tgt, corr, keep = E.few_finite_case(k)
        P, Q, finite = R.pair_points(src, tgt, corr)
        assert len(corr) == 500 and finite.sum() == k and (np.flatnonzero(finite) == keep).all()
        assert np.isnan(src).any() and np.isinf(tgt).any()


def test_min_sample_distance_where_d2_overflows(api):
    r, src, tgt, corr, true, prm = E.reference("min_sample_distance_inf_d2")
    P, Q, finite = R.pair_points(src, tgt, corr)
    msd = prm["min_sample_distance"]
    tries, inf_samples, finite_samples = [], 0, 0
    for h in range(r.iterations):
        T, ids, t = R.hypothesis(api, P, Q, finite, prm["seed"], h, msd)
        tries.append(t)
        if t < 0:
            continue
        d2 = [float(R.l2_simple(P[ids[a]], P[ids[b]])) for a, b in ((0, 1), (0, 2), (1, 2))]
        assert all(d > msd * msd for d in d2)
        inf_samples += any(np.isinf(d) for d in d2)
        finite_samples += all(np.isfinite(d) for d in d2)
    print("min_sample_distance at 2^62: tries", tries, "samples with a +inf d2", inf_samples, "all finite", finite_samples)
    assert r.found and sum(t > 0 for t in tries) > 5 and sum(t >= 0 for t in tries) > 10 and inf_samples > 3 and finite_samples > 3
    # the same decisions as at scale 1 with 2.5: +inf stands for "more than 4 apart"
    one = R.sac(api, *E.scale_base()[:3], **dict(E.scale_prm(0), min_sample_distance=2.5, seed=prm["seed"]))
    assert (one.sample, one.best_hypothesis, one.iterations, one.n_inliers) == (r.sample, r.best_hypothesis, r.iterations, r.n_inliers)
    r, src, tgt, corr, true, prm = E.reference("min_sample_distance_1e200")
    assert prm["min_sample_distance"] * prm["min_sample_distance"] == math.inf and not r.valid.any() and not r.found and r.iterations == 1
