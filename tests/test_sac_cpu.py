"""The pose-from-correspondences contract without a GPU: the reference of tests/sac_ref.py against known answers, a literal
RANSAC loop and a case with a known motion; the host-only rules of csrc/sac_plan.hpp through their stand-alone program; and what
every case of tests/sac_cases.py is FOR, asserted on the reference, so that the GPU tests compare bits on cases that reach the
branches they name.
"""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import sac_cases as K
import sac_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api(rs):
    from rsreg_amd import api
    return api


def test_generator_known_answers():
    """The finaliser is splitmix64's: with seed 0 the counters 1, 2, 3 (h = 0, draws 1 .. 3) give the published first outputs of
    splitmix64 seeded with 0.  The index is the high word of (high word of z) * n; the literals below were worked out by hand
    from those outputs: 0xE220A839 = 3 793 791 033, times 1000, over 2^32 = 883.3 -> 883; 0x6E789E6A -> 431.5 -> 431; 0x06C45D18 ->
    26.4 -> 26."""
    published = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)
    for d, z in zip((1, 2, 3), published):
        assert int(R.draw_index(0, 0, d, 1 << 32)) == z >> 32            # n = 2^32: the index IS the high word
        assert int(R.draw_index(0, 0, d, 1000)) == ((z >> 32) * 1000) >> 32
    assert [int(R.draw_index(0, 0, d, 1000)) for d in (1, 2, 3)] == [883, 431, 26]
    # the counter is 64 * h + draw, the seed is added to the product, everything wraps modulo 2^64
    assert int(R.draw_index(0, 1, 0, 1 << 32)) == int(R.draw_index(0, 0, 64, 1 << 32))
    assert int(R.draw_index(K_GOLDEN, 0, 0, 1 << 32)) == published[0] >> 32
    assert int(R.draw_index((1 << 64) - K_GOLDEN, 0, 3, 1 << 32)) == published[1] >> 32
    # an array of hypotheses at once gives what one at a time gives; every index is below n
    hs = np.arange(500)
    for n in (1, 2, 3, 1000, (1 << 31) - 17):
        got = R.draw_index(12345, hs, 7, n)
        assert (got < n).all() and [int(g) for g in got[:20]] == [int(R.draw_index(12345, int(h), 7, n)) for h in hs[:20]]
    # ... and spreads: 3 000 draws over 10 cells, every cell within 25 % of its share
    assert (np.abs(np.bincount(R.draw_index(9, np.arange(3000), 0, 10).astype(np.int64), minlength=10) - 300) < 75).all()


K_GOLDEN = 0x9E3779B97F4A7C15


def _literal_ransac(counts, n, probability, max_iterations, valid):
    """pcl::RandomSampleConsensus::computeModel as a plain loop over precomputed counts (written apart from sac_ref.replay: a for
    loop with a break, k updated through the same three lines of ransac.hpp)"""
    best, winner, k, iterations = -(2 ** 31 - 1), -1, 1.0, 0
    for h in range(max_iterations):
        if not h < k:
            break
        iterations = h + 1
        c = int(counts[h])
        if not valid[h] or c <= best:
            continue
        best, winner = c, h
        w = best / n
        p_no_outliers = 1.0 - w * w * w
        p_no_outliers = max(np.finfo(np.float64).eps, p_no_outliers)
        p_no_outliers = min(1.0 - np.finfo(np.float64).eps, p_no_outliers)
        k = math.log(1.0 - probability) / math.log(p_no_outliers)
    return max(best, -1), winner, iterations


def test_replay_equals_a_literal_loop():
    rng = np.random.default_rng(3)
    stopped_early = ran_out = 0
    for trial in range(300):
        n = int(rng.integers(3, 3000))
        max_it = int(rng.integers(0, 400))
        counts = rng.integers(0, max(2, n // int(rng.integers(1, 40))), 400)
        if trial % 3 == 0:
            counts[int(rng.integers(0, 400))] = n                 # every pair an inlier: k = log(1 - p) / log(eps)
        p = float(rng.choice([0.5, 0.9, 0.99, 0.999999]))
        valid = rng.uniform(size=400) < float(rng.choice([0.02, 0.7, 1.0]))
        got = R.replay(counts, n, p, max_it, check_margin=False, valid=valid)
        assert got[:3] == _literal_ransac(counts, n, p, max_it, valid), (trial, n, max_it, p)
        stopped_early += got[2] < max_it
        ran_out += got[2] == max_it
    assert stopped_early > 50 and ran_out > 50
    assert R.replay([0, 0, 0], 10, 0.99, 5, valid=[False] * 3)[:3] == (-1, -1, 1)    # no valid hypothesis: k stays 1, one hypothesis consumed
    assert R.replay([0, 0, 0, 0, 0], 10, 0.99, 5)[:3] == (0, 0, 5)                   # a valid one without an inlier sets k: on to max_iterations
    assert R.replay([5], 10, 0.99, 0)[:3] == (-1, -1, 0)


def _independent_outlier_inliers(src, tgt, corr, true, threshold):
    """indices of the pairs that are NOT true pairs and still lie within the threshold of the motion, in float64 -- and a check that
    none of them, and no true pair, is near enough to the threshold for float32 rounding to matter"""
    moved = src[corr["index_query"]].astype(np.float64) @ K.MOTION[:3, :3].T + K.MOTION[:3, 3]
    d = np.linalg.norm(moved - tgt[corr["index_match"]].astype(np.float64), axis=1)
    assert (np.abs(d - threshold) > 1e-4).all() and (d[true] < 1e-5).all()
    return np.flatnonzero(~true & (d < threshold))


def test_reference_recovers_the_known_motion(api):
    src, tgt, corr, true = K.motion_case(2000, 0.4, 1)
    assert len(corr) == 2000 and true.sum() == 800
    r = R.sac(api, src, tgt, corr, **K.SAC_CASES["first_batch"][1])
    assert r.found and np.linalg.norm(r.transform.astype(np.float64) - K.MOTION) < 1e-4
    lucky = _independent_outlier_inliers(src, tgt, corr, true, 0.05)
    want = np.sort(np.concatenate([np.flatnonzero(true), lucky]))
    assert (np.flatnonzero(r.flags) == want).all() and r.n_inliers == len(want)
    assert (r.kept == corr[want]).all()                                # input order, records unchanged (distance included)
    assert true[list(r.sample)].all() and len(set(r.sample)) == 3
    # the winner is the FIRST hypothesis with the final best, and the replay stopped on k, not on max_iterations
    assert r.counts[r.best_hypothesis] == r.n_inliers and (r.counts[:r.best_hypothesis] < r.n_inliers).all()
    assert r.best_hypothesis < r.iterations < 1000 and r.iterations == max(math.ceil(r.ks[-1]), r.best_hypothesis + 1)


@pytest.fixture(scope="module")
def refs(api):
    out = {}
    for name, (make, prm) in K.SAC_CASES.items():
        src, tgt, corr, true = make()
        out[name] = (R.sac(api, src, tgt, corr, **prm), src, tgt, corr, true, prm)
    return out


def test_cases_reach_the_branches_they_are_named_for(api, refs):
    """(the k-margin condition -- every k the replay computes at least 1e-9 * k away from an integer -- is asserted inside
    sac_ref.replay for every one of these cases)"""
    r = refs["first_batch"][0]
    assert r.found and r.iterations < K.FIRST_BATCH
    r = refs["later_batch"][0]
    assert r.found and K.FIRST_BATCH < r.iterations < 2000 and r.best_hypothesis >= 0
    r = refs["to_max_iterations"][0]
    assert r.found and r.iterations == 300 and r.ks[-1] > 300
    for name in ("repeated_sources", "min_sample_distance", "nonfinite"):
        r, src, tgt, corr, true, prm = refs[name]
        P, Q, finite = R.pair_points(src, tgt, corr)
        tries = [R.hypothesis(api, P, Q, finite, prm["seed"], h, prm.get("min_sample_distance", 0.0))[2] for h in range(200)]
        assert r.found and sum(t > 0 for t in tries) > (20 if name != "nonfinite" else 3), (name, tries[:20])
        if name == "min_sample_distance":
            assert sum(t < 0 for t in tries) > 5 and sum(t >= 0 for t in tries) > 50      # some hypotheses run out of tries, most do not
            i = list(r.sample)
            assert min(np.linalg.norm(P[i[a]] - P[i[b]]) for a, b in ((0, 1), (0, 2), (1, 2))) > 3.2
        if name == "nonfinite":
            assert (~finite).sum() >= 7 and not r.flags[~finite].any() and (true & ~finite).any()
    r, src, tgt, corr, true, prm = refs["all_invalid"]
    assert not r.found and r.iterations == 1 and (r.counts == 0).all() and (r.transform == np.eye(4)).all() and len(r.kept) == len(corr)
    r = refs["two_pairs"][0]
    assert not r.found and r.iterations == 0 and len(r.kept) == 2


def test_threshold_pairs_sit_on_both_sides():
    both = set()
    for thr in (0.05, 0.07, 1.5):
        src, tgt, corr, d2 = K.threshold_pairs(thr)
        f = np.float32(thr * thr)
        assert sorted(set(d2.tolist())) == [float(np.nextafter(f, np.float32(0))), float(f), float(np.nextafter(f, np.float32(np.inf)))]
        P, Q, finite = R.pair_points(src, tgt, corr)
        got = R.within(np.eye(4, dtype=np.float32), P, Q, finite, thr)
        assert (got == (d2.astype(np.float64) < thr * thr)).all() and got[:8].all() and not got[16:].any()
        both.add(bool(got[8:16].all()))                               # d2 == (float)(thr^2): inside iff the cast rounded DOWN
        assert got[8:16].all() or not got[8:16].any()
    assert both == {True, False}


def test_sum_tree_depth():
    assert R.sum_tree_depth(1) == 17 and R.sum_tree_depth(128 * 256) == 17 and R.sum_tree_depth(128 * 256 + 1) == 18


def test_plan_rule_covers_every_cell_once():
    """csrc/sac_plan.hpp through tests/cpp/sac_plan_rule.cpp, compiled with the sanitizers: the constants the cases mirror, the plan
    against its Python twin, every (tile, chunk) cell owned by exactly one workgroup, the workgroup count bounded, the batches."""
    sizes = [(n, H) for n in K.PAIR_COUNTS + (1 << 20, (1 << 31) - 17) for H in K.HYP_COUNTS + K.HYP_SLICE_EDGE + (1, 1 << 20)]
    cover = [(n, H) for n, H in sizes if -(-n // K.TILE) * -(-H // K.CHUNK) <= 1 << 22]
    max_its = (0, 1, 255, 256, 257, 768, 769, 1000, 7936, 7937, 20000)
    lines = ["plan %d %d" % s for s in sizes] + ["cover %d %d" % s for s in cover] + ["batches %d" % m for m in max_its]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sac_plan_rule")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                            os.path.join(ROOT, "tests", "cpp", "sac_plan_rule.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stdout[-3000:]
    out = r.stdout.strip().splitlines()
    assert out[0].split() == ["constants"] + [str(v) for v in (K.BLOCK, K.PAIRS_PER_LANE, K.TILE, K.CHUNK, K.MAX_GROUPS, K.FIRST_BATCH, K.MAX_BATCH, K.TRIES)]
    assert R.TRIES == K.TRIES and K.TILE == K.BLOCK * K.PAIRS_PER_LANE and len(out) == 1 + len(lines)
    grown = 0
    for line, want in zip(out[1:], lines):
        v = line.split()
        assert v[:len(want.split())] == want.split()
        if v[0] == "plan":
            n, H, tiles, chunks, per, slices = (int(x) for x in v[1:])
            assert (tiles, chunks, per, slices) == K.plan(n, H)
            assert tiles == -(-n // K.TILE) and chunks == -(-H // K.CHUNK) and 1 <= per <= chunks
            assert (slices - 1) * per < chunks <= slices * per                     # the slices tile the chunks, none is empty
            assert tiles * slices <= K.MAX_GROUPS + tiles < 2 ** 31                # bounded: one launch dimension holds the grid
            assert per == 1 or tiles * slices > K.MAX_GROUPS // 2                  # a slice grows only to keep that bound
            grown += per > 1
        elif v[0] == "cover":
            n, H, groups, bad = (int(x) for x in v[1:])
            tiles, chunks, per, slices = K.plan(n, H)
            assert groups == tiles * slices and bad == 0, line
        else:
            m, got = int(v[1]), [int(x) for x in v[2:]]
            want_b, done = [], 0
            while K.batch(done, m):
                want_b.append(K.batch(done, m))
                done += want_b[-1]
            assert got == want_b and sum(got) == m and all(b <= K.MAX_BATCH for b in got)
            assert got[:5] == [256, 512, 1024, 2048, 4096][:len(got[:5])] or sum(got[:5]) == m
    assert grown >= 5 and K.plan(3, K.HYP_SLICE_EDGE[1])[2] == 1 and K.plan(3, K.HYP_SLICE_EDGE[2])[2] == 2
