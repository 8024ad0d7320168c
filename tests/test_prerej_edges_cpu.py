"""What every case of tests/prerej_edge_cases.py is FOR, asserted on the reference (tests/prerej_ref.py) without a GPU, so that
tests/test_prerej_edges_gpu.py compares bits on cases that are proven to reach the branch they name: a winner in the second round of
hypotheses and a last round of one, transforms scored past a round, a batch cap below 256, degenerate samples, and -- from the
reference's own float32 edge lengths (prerej_ref.sample_edges) -- where in the float32 range the polygon test of a scaled cloud is
decided.

The whole file takes 7 s on one core (measured), 4.5 s of them the three references of the three-round case and 1.4 s the source
of 8 193 tiles.
"""
import math

import numpy as np
import pytest

import prerej_cases as C
import prerej_edge_cases as X
import prerej_ref as R
import sac_ref as S


@pytest.fixture(scope="module")
def api(rs):
    from rsreg_amd import api
    return api


def _pair_d2(xyz):
    """(n, n) float32: the L2_Simple squared distance of every two records"""
    return S.l2_simple(xyz[:, None, :], xyz[None, :, :])


def _distinct_samples(name):
    """[(h, its three source records)] of the hypotheses of a case that draw three distinct records"""
    src, tgt, nbr, prm = X.CASES[name]
    out = []
    for h in range(prm["max_iterations"]):
        ids = tuple(int(S.draw_index(prm["seed"], h, d, len(src))) for d in range(3))
        if len(set(ids)) == 3:
            out.append((h, ids))
    return out


# ---- A. rounds and batches
def test_rounds_full_call(api):
    late, early, by_inliers = (X.reference(n) for n in ("rounds_winner_in_round_2", "rounds_winner_in_round_1", "rounds_by_inliers"))
    for name, r in (("rounds_winner_in_round_2", late), ("rounds_winner_in_round_1", early), ("rounds_by_inliers", by_inliers)):
        src, tgt, nbr, prm = X.CASES[name]
        assert prm["max_iterations"] == 2 * X.ROUND + 1 == len(r.valid) and (nbr[np.arange(40) % 4 != 0] == -1).all() and (nbr[::4] >= 0).all()
        assert r.found and r.valid[:X.ROUND].any() and r.valid[X.ROUND:2 * X.ROUND].any() and r.n_valid == r.valid.sum()
        print(name, "winner", r.best_hypothesis, "valid a round", r.valid[:X.ROUND].sum(), r.valid[X.ROUND:2 * X.ROUND].sum(), r.valid[2 * X.ROUND:].sum())
    assert X.ROUND <= late.best_hypothesis < 2 * X.ROUND and early.best_hypothesis < X.ROUND
    assert by_inliers.best_hypothesis >= X.ROUND and (by_inliers.counts == late.counts).all()
    # the second round's winner had something to beat: a hypothesis of the first round qualifies as well
    assert (late.valid[:X.ROUND] & (late.counts[:X.ROUND] > 0)).any()


def test_score_past_a_round():
    src, tgt, Ts, pick, rng = X.score_past_a_round()
    counts, sums = X.distinct_scores("past_a_round")
    assert len(pick) == X.ROUND + 17 and len(Ts) == 12 and len(src) == 129 and len(tgt) == 300 and pick.min() == 0 and pick.max() == 11
    three = pick[[X.ROUND - 1, X.ROUND, X.ROUND + 16]]
    assert len(set(three.tolist())) == 3 and len(set(counts[three].tolist()) - {0}) >= 2, (three, counts[three])
    assert len(np.unique(Ts.reshape(12, -1).view(np.uint32), axis=0)) == 12                      # the 12 are distinct


def test_batch_cap_below_256():
    src, tgt, Ts, pick, rng = X.batch_cap_below_256()
    n = len(src)
    assert n == 128 * 8193 == 1048704 and C.plan(n, 255)[0] == 8193 and C.batch_cap(n) == 255 and C.batch_cap(n - 128) == 256
    assert len(pick) == 256 and len(tgt) == 5 and np.isnan(Ts[X.CAP_NAN]).any() and np.isfinite(np.delete(Ts, X.CAP_NAN, axis=0)).all()
    three = pick[[0, 254, 255]]
    assert len(set(three.tolist())) == 3 and X.CAP_NAN not in three, three
    counts, sums = X.distinct_scores("cap")
    assert 0.01 * n < counts[0] < 0.99 * n and counts[X.CAP_NAN] == 0 and sums[X.CAP_NAN] == 0.0 and len(set(counts.tolist())) == 4
    assert (Ts[0] == C.TURN.astype(np.float32)).all()
    # the reference's own tree, 8 193 groups deep, against the exact sum of the TURN row's inlier d2
    count, total, flags, d2 = R.score(Ts[0], src, tgt, rng)
    terms = d2[flags].astype(np.float64)
    exact = math.fsum(terms)
    assert (count, total) == (counts[0], sums[0]) and R.sum_tree_depth(n) == 6 + 1 + 8192
    assert abs(total - exact) <= R.sum_tree_depth(n) * 2.0 ** -53 * exact, (total, exact)


# ---- B. degenerate samples
def test_sources_of_one_to_four_records(api):
    for n in (1, 2):
        r = X.reference("ns_%d" % n)
        assert len(X.CASES["ns_%d" % n][0]) == n and r.n_valid == 0 and not r.found and r.sample == (-1, -1, -1)
        assert not _distinct_samples("ns_%d" % n)
    r = X.reference("ns_3")
    drawn = _distinct_samples("ns_3")
    assert 0 < r.n_valid < 128 and r.found and r.n_inliers == 3 and sorted(r.sample) == [0, 1, 2]
    assert r.n_valid == len(drawn) == 31                                                         # six draws of 27 are three distinct records: 128 * 6 / 27 = 28
    r = X.reference("ns_4")
    assert r.found and r.n_inliers == 4 and r.n_valid == len(_distinct_samples("ns_4")) == 49


def test_ties_first_wins(api):
    for rule in (0, 1):
        name = "ties_first_wins_rule_%d" % rule
        src, tgt, nbr, prm = X.CASES[name]
        r = X.reference(name)
        assert prm["select_by_inliers"] == rule and len(src) == 4 and r.found and r.n_inliers == 4
        w = r.best_hypothesis
        tied = [h for h in np.flatnonzero(r.valid) if r.counts[h] == r.counts[w] and np.float64(r.sums[h]).tobytes() == np.float64(r.sums[w]).tobytes()]
        same_sample = [h for h in np.flatnonzero(r.valid) if R.hypothesis(api, src, tgt, nbr, prm["seed"], int(h), 0.9)[1:] == (r.sample, r.match)]
        print(name, "winner", w, "equal (count, sum)", tied, "same sample in the same order", same_sample)
        assert tied == [24, 39, 42, 74, 80] and same_sample == [24, 74]
        assert w == min(tied) == min(same_sample) and max(tied) > w and max(same_sample) > w
        # nothing else beats the tied ones: the winner is decided by "the first wins" alone
        assert all(r.sums[h] / r.counts[h] >= r.fitness for h in np.flatnonzero(r.valid))


def test_collinear_sources(api):
    src, tgt, nbr, prm = X.CASES["collinear_sources"]
    a, b, c = (src[i].astype(np.float64) for i in (0, 1, 2))
    for p in src.astype(np.float64):
        assert (np.cross(b - a, p - a) == 0).all()                                                # collinear exactly (float64 is exact on these dyadic numbers)
    ds, dt = _pair_d2(src), _pair_d2(tgt)
    off = ~np.eye(len(src), dtype=bool)
    assert (ds == dt).all() and (ds[off] > 0).all() and prm["similarity_threshold"] == X.JUST_UNDER_ONE < 1.0      # every edge ratio is exactly 1: every triple passes
    for h, e in X.edges("collinear_sources").items():
        assert (e[:, 2] == 1.0).all()
    r = X.reference("collinear_sources")
    # the host solve accepts a rank-1 sample (it completes the basis): every hypothesis of three distinct records is valid, 120 of 128
    assert r.n_valid == len(_distinct_samples("collinear_sources")) == 120 and r.found and r.n_inliers == 60


def test_coincident_sources(api):
    src = X.CASES["coincident_sources_sim_0.9"][0]
    assert len(src) == 40 and (src[0::2] == src[1::2]).all()
    for sim in (0.9, 0.0):
        name = "coincident_sources_sim_%g" % sim
        r = X.reference(name)
        assert X.CASES[name][3]["similarity_threshold"] == sim
        twins = [h for h, ids in _distinct_samples(name) if len({i // 2 for i in ids}) < 3]
        assert len(twins) >= 3 and not r.valid[twins].any() and r.n_valid > 0 and r.found
        for h in twins:                                                                           # 0 / 0: a NaN sim on the twins' edge
            e = X.edges(name)[h]
            assert ((e[:, 0] == 0) & (e[:, 1] == 0) & np.isnan(e[:, 2])).sum() == 1
        assert r.n_valid == len(_distinct_samples(name)) - len(twins) == 106


def test_one_target_record(api):
    r = X.reference("one_target_record_sim_0.9")
    assert (X.CASES["one_target_record_sim_0.9"][2] == 7).all() and r.n_valid == 0 and not r.found
    r = X.reference("one_target_record_sim_0")
    drawn = _distinct_samples("one_target_record_sim_0")
    for h, ids in drawn:                                                                          # dt is 0 on every edge, ds is not: 0 / ds = 0 >= 0 passes
        e = X.edges("one_target_record_sim_0")[h]
        assert (e[:, 1] == 0).all() and (e[:, 0] > 0).all() and (e[:, 2] == 0).all()
    # the host solve accepts the rank-0 sample (a turn it completes by its own rule, the translation onto record 7): every hypothesis of
    # three distinct records is valid, 123 of 128, and at most the source records next to the sample's centroid are inliers
    assert r.n_valid == len(drawn) == 123 and r.found and r.match == (7, 7, 7) and r.n_inliers == 1


def test_mirrored_target(api):
    src, tgt, nbr, prm = X.CASES["mirrored_target"]
    assert (tgt == src * np.float32([1, 1, -1])).all() and (_pair_d2(src) == _pair_d2(tgt)).all()            # every edge ratio is 1: every triple passes
    r = X.reference("mirrored_target")
    assert r.n_valid == len(_distinct_samples("mirrored_target")) == 120 and r.found
    T = r.transform.astype(np.float64)
    assert abs(np.linalg.det(T[:3, :3]) - 1) < 1e-5                                              # a proper rotation fits the triple, not the mirror
    assert set(r.sample) <= set(r.inliers.tolist()) and 3 <= r.n_inliers < len(src) // 4


def test_same_cloud(api):
    src, tgt, nbr, prm = X.CASES["same_cloud"]
    r = X.reference("same_cloud")
    held = (nbr[:, 0] == np.arange(60)).mean()
    assert tgt is src and 0.5 < held < 0.9 and r.found and r.n_inliers == len(src) == 60 and 0 < r.n_valid < 128
    assert np.abs(r.transform.astype(np.float64) - np.eye(4)).max() < 1e-6                       # (float32 rounding of a pose in the unit box)


# ---- C. the float32 range
def _all_edges(name):
    e = X.edges(name)
    return np.concatenate([e[h] for h in sorted(e)]) if e else np.zeros((0, 3), np.float32)


def test_scaled_clouds(api):
    for e in X.SCALE_EXPONENTS:
        name = "scale_2^%+d" % e
        r, edges = X.reference(name), _all_edges(name)
        assert len(edges) == 3 * 60                                                               # 60 of the 64 hypotheses draw three distinct records
        print(name, "n_valid", r.n_valid, "inliers", r.n_inliers, "ds: zero %d, denormal %d, inf %d" %
              ((edges[:, 0] == 0).sum(), ((edges[:, 0] > 0) & (edges[:, 0] < X.FLT_MIN)).sum(), np.isinf(edges[:, 0]).sum()))
        if e in (-70, -62, -30, 30, 62):
            assert r.n_valid == 60 and r.found and r.n_inliers == 60
        else:
            assert r.n_valid == 0 and not r.found and np.isnan(edges[:, 2]).all()
        if e == -70:
            low = (edges[:, :2] > 0) & (edges[:, :2] < X.FLT_MIN)
            assert low.all()                                                                      # every ds and dt is a positive denormal: the division decides all of them
        if e == -100:
            assert (edges[:, :2] == 0).all()
        if e in (70, 100):
            assert np.isposinf(edges[:, :2]).all()
    for e in (-70, 62):
        name = "scale_2^%+d_random_rows" % e
        r, edges = X.reference(name), _all_edges(name)
        fails = (edges[:, 2] < np.float32(0.9) * np.float32(0.9)).sum()
        assert 0 < r.n_valid < 60 and fails > 20 and r.found and r.n_inliers == 60 and np.isfinite(edges).all()
        if e == -70:
            assert (edges[:, 0] > 0).all() and (edges[:, :2] < X.FLT_MIN).all()                  # denormals (a dt of 0: two random rows name one target record)
    # a valid pose at 2^62 throws part of the source out of the float range: some d2 of a scored hypothesis is +inf
    src, tgt, nbr, prm = X.CASES["scale_2^+62_random_rows_sim_0"]
    r = X.reference("scale_2^+62_random_rows_sim_0")
    assert prm["similarity_threshold"] == 0.0 and r.n_valid > 50 and r.counts[r.valid].min() < 10 and r.n_inliers == 60
    top = 0.0
    for h in np.flatnonzero(r.valid):
        T = R.hypothesis(api, src, tgt, nbr, prm["seed"], int(h), 0.0)[0]
        d2 = R.score(T, src, tgt, prm["max_correspondence_distance"])[3]
        assert np.isfinite(d2).all()
        top = max(top, float(d2.max()))
    print("scale_2^+62_random_rows_sim_0: valid %d, counts %s, the largest nearest d2 2^%.1f" % (r.n_valid, sorted(set(r.counts[r.valid].tolist())), math.log2(top)))
    # a rigid pose keeps the cloud within a few 2^62 of the target, so a nearest d2 stays finite -- but it is of the box's own size
    # squared, 2^123 here, 2^5 below FLT_MAX (+inf itself is reached by the transforms of thrown_out_of_range)
    assert top > 2.0 ** 122
    assert np.abs(r.transform[:3, 3]).max() > 2.0 ** 60 and np.abs(X.reference("scale_2^-62").transform[:3, 3]).max() < 2.0 ** -60


def test_denormal_cloud(api):
    src, tgt, nbr, prm = X.CASES["denormal_cloud"]
    assert (src > 0).all() and (src < X.FLT_MIN).all() and (tgt > 0).all() and (tgt < X.FLT_MIN).all()
    r, edges = X.reference("denormal_cloud"), _all_edges("denormal_cloud")
    # every squared edge underflows to 0: 0 / 0, nothing is valid
    assert len(edges) == 180 and (edges[:, :2] == 0).all() and np.isnan(edges[:, 2]).all() and r.n_valid == 0 and not r.found


def test_range_at_a_float():
    pairs = X.range_pairs()
    want = [0.0, 2.0 ** -149, 2.0 ** -148, 0.0625, 0.875, float(np.nextafter(np.float32(2.0 ** 127), np.float32(0))), math.inf]
    assert [float(d2) for _, _, _, d2 in pairs] == want and all(d2.dtype == np.float32 for _, _, _, d2 in pairs)
    a, b, c = X.BIG_D_ABC
    assert a * a + b * b + c * c == 2 * (2 ** 24 - 1) and all(float(np.float32(v)) == v for v in (a * a, b * b, a * a + b * b))
    eye = np.eye(4, dtype=np.float32)
    calls = 0
    for label, s, t, d2 in pairs:
        assert len(s) == 1 and len(t) in (1, 2)
        for rng in X.FIXED_RANGES:
            assert R.score(eye, s, t, rng)[0] == int(float(d2) < rng * rng), (label, rng)
            calls += 1
        if not np.isfinite(d2):
            assert [R.score(eye, s, t, rng)[0] for rng in X.FIXED_RANGES] == [0] * 5
            continue
        out, inside = X.ranges_around(d2)
        root = math.sqrt(float(d2))
        if root * root == float(d2):                                                             # sqrt(d2) is exact in double: AT it, not an inlier
            assert out[0] == root
        assert label not in ("0", "2^-148", "0.0625") or out[0] == root
        assert inside[0] == np.nextafter(out[0], math.inf) or d2 == 0
        for rng in out:
            assert R.score(eye, s, t, rng)[0] == 0, (label, rng)
        for rng in inside:
            assert R.score(eye, s, t, rng)[0] == 1, (label, rng)
        calls += len(out) + len(inside)
    assert 50 <= calls <= 70
    assert [int(float(pairs[0][3]) < r * r) for r in X.FIXED_RANGES] == [0, 0, 1, 1, 1]         # d2 = 0: 1e-200 squares to 0 as well
    assert [int(float(pairs[5][3]) < r * r) for r in X.FIXED_RANGES] == [0, 0, 0, 1, 1]         # below 2^127: 2e19 squares to 4e38, above FLT_MAX


def test_thrown_out_of_range():
    src, tgt, Ts = X.thrown_out_of_range()
    assert len(Ts) == 14 and np.abs(src).max() > 2.0 ** 61 and (np.abs(Ts) == np.finfo(np.float32).max).any()
    counts, sums = R.score_transforms(Ts, src, tgt, X.THROWN_RANGES[0])
    print("thrown out of range: counts", counts.tolist())
    assert len(set(counts.tolist())) >= 3 and (counts == 0).any() and (counts == 60).any()
    finite, _ = R.score_transforms(Ts, src, tgt, X.THROWN_RANGES[1])
    assert X.THROWN_RANGES[1] * X.THROWN_RANGES[1] == math.inf and (finite >= counts).all() and set(finite.tolist()) == {0, 60}
