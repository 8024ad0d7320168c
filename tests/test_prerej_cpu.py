"""The pose-from-descriptor-neighbours contract (rsreg_cloud_score_transforms, rsreg_cloud_prerejective) without a GPU: the reference
of tests/prerej_ref.py against what can be stated on its own, the host-only rules of csrc/prerej_plan.hpp through their stand-alone
program, and what the cases of tests/prerej_cases.py are FOR, asserted on the reference, so that the GPU tests compare bits on cases
that reach the branches they name.

The argument checks of the two entry points need a context, and a context needs a device: they are in tests/test_prerej_gpu.py
(test_refusals), marked gpu.
"""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import prerej_cases as C
import prerej_ref as R
import sac_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api(rs):
    from rsreg_amd import api
    return api


@pytest.fixture(scope="module")
def refs(api):
    return {name: R.prerejective(api, src, tgt, nbr, **prm) for name, (src, tgt, nbr, prm) in C.PREREJ_CASES.items()}


@pytest.mark.parametrize("n", (1, 63, 64, 65, 127, 128, 129, 300, 1000))
def test_sum_tree_within_its_depth_bound(n):
    """each addition rounds once and every partial sum is bounded by sum|terms|: |tree - exact| <= depth * 2^-53 * sum|terms|
    (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., §4.2), depth = prerej_ref.sum_tree_depth(n)"""
    rng = np.random.default_rng(n)
    terms = (rng.random(n) * rng.choice([1e-6, 1.0, 1e4], n)).astype(np.float32).astype(np.float64)
    terms[rng.random(n) < 0.3] = 0.0
    got, exact = R.sum_tree(terms), math.fsum(terms)
    assert abs(got - exact) <= R.sum_tree_depth(n) * 2.0 ** -53 * math.fsum(np.abs(terms)), (got, exact)
    # the order is the contract's: one group is its two waves' pairwise trees, then the groups one after the other
    if n <= 128:
        v = np.zeros(128)
        v[:n] = terms
        w = []
        for half in (v[:64], v[64:]):
            t = half.copy()
            while len(t) > 1:
                t = t[:len(t) // 2] + t[len(t) // 2:]
            w.append(t[0])
        assert got == w[0] + w[1]
    assert R.sum_tree([]) == 0.0 and R.sum_tree_depth(128) == 7 and R.sum_tree_depth(129) == 8


def test_nearest_distance_by_brute_force():
    tgt = np.float32([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 3, 4]])
    q = np.float32([[0.25, 0, 0], [0.75, 0, 0], [0, 3, 3], [np.inf, 0, 0], [100, 0, 0]])
    got = R.nearest_d2(q, tgt)
    assert got.dtype == np.float32 and got.tolist() == [0.0625, 0.0625, 1.0, np.inf, 99.0 * 99.0]
    assert np.isinf(R.nearest_d2(q, tgt[2:3])).all() and np.isinf(R.nearest_d2(q, tgt[:0])).all()


def test_true_pairs_pass_the_polygon_test_and_score_every_point(api):
    src, tgt, true_of = C.pair(120, 3)
    nbr = true_of.reshape(-1, 1)
    hits = 0
    for h in range(40):
        T, ids, match = R.hypothesis(api, src, tgt, nbr, 5, h, 0.9)
        if len(set(ids)) < 3:
            assert T is None
            continue
        assert T is not None and tuple(true_of[list(ids)]) == match and R.polygon_ok(src[list(ids)], tgt[list(match)], 0.9)
        count, total, flags, d2 = R.score(T, src, tgt, C.RANGE)
        assert count == len(src) and flags.all() and total / count < 1e-10
        assert np.linalg.norm(T.astype(np.float64) - C.TURN) < 1e-4
        hits += 1
    assert hits > 30
    # the strict compare: a record AT the range is not an inlier
    one = np.float32([[0, 0, 0]])
    eye = np.eye(4, dtype=np.float32)
    assert R.score(eye, one, np.float32([[0.5, 0, 0]]), 0.5)[0] == 0 and R.score(eye, one, np.float32([[0.5, 0, 0]]), 0.5000001)[0] == 1
    assert R.score(eye, one, one, 0.0)[0] == 0 and R.score(eye, one, one, 1e-30)[0] == 1


def test_polygon_test_edges():
    tri = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    assert R.polygon_ok(tri, tri + np.float32(2), 0.999) and R.polygon_ok(tri, tri * np.float32(0.96), 0.9)
    # squared lengths against the squared threshold: the edges' LENGTHS may differ by the threshold's factor, 0.9, and no more
    assert R.polygon_ok(tri, tri * np.float32(0.91), 0.9) and not R.polygon_ok(tri, tri * np.float32(0.89), 0.9)
    assert R.polygon_ok(tri * np.float32(0.91), tri, 0.9) and not R.polygon_ok(tri * np.float32(0.89), tri, 0.9)
    assert R.polygon_ok(tri, tri * np.float32(100), 0.0)
    same = np.float32([[0, 0, 0], [0, 0, 0], [0, 1, 0]])
    assert not R.polygon_ok(same, same, 0.0)                                       # 0 / 0 is NaN, which fails at any threshold


def test_selection_rules(refs):
    counts, sums, valid = [5, 9, 9, 3, 0, 7], [0.5, 0.9, 0.45, 0.03, 0.0, 0.07], [True, True, True, True, True, False]
    assert R.select(counts, sums, valid, 10) == (3, 0.03 / 3)                       # PCL: the lowest error, whatever the count
    assert R.select(counts, sums, valid, 10, 0.0, 1) == (2, 0.45 / 9)               # the highest count, then the lowest error
    assert R.select(counts, sums, valid, 10, 0.5) == (2, 0.05)                      # 5 / 10 AT the bound qualifies, and ties go to the first
    assert R.select(counts, sums, valid, 10, 0.5000001)[0] == 2 and R.select(counts, sums, valid, 10, 0.95)[0] == -1
    assert R.select([4, 4], [0.4, 0.4], [True, True], 4, 1.0, 1)[0] == 0 and R.select([0], [0.0], [True], 4)[0] == -1
    # the case built for it: the two rules pick different hypotheses
    a, b = refs["decoy_pcl_rule"], refs["decoy_by_inliers"]
    assert a.found and b.found and a.best_hypothesis != b.best_hypothesis
    assert a.n_inliers == 6 and set(a.sample) <= set(range(6)) and b.n_inliers == 12 and set(b.sample) <= set(range(6, 12))
    assert a.fitness < 1e-12 < b.fitness and (a.counts == b.counts).all() and (a.sums == b.sums).all()


def test_cases_reach_the_branches_they_are_named_for(refs):
    for k in (1, 2, 5, 16):
        r = refs["k_%d" % k]
        src, tgt, nbr, prm = C.PREREJ_CASES["k_%d" % k]
        assert nbr.shape[1] == k and (nbr[[0, 7, 64]] == -1).all() and r.found and 0 < r.n_valid < prm["max_iterations"]
    for name in ("all_ineligible", "polygon_always_fails"):
        r = refs[name]
        assert not r.found and r.n_valid == 0 and r.best_hypothesis == -1 and r.sample == (-1, -1, -1) and (r.transform == np.eye(4)).all()
    assert refs["similarity_zero"].n_valid > 55                                    # every sample of three distinct eligible records is scored
    r = refs["similarity_just_under_one"]
    assert r.found and r.n_inliers == 60 and r.fitness == 0.0 and r.n_valid > 30
    assert refs["fraction_0"].found and refs["fraction_half"].found and refs["fraction_0"].best_hypothesis != refs["fraction_half"].best_hypothesis
    assert refs["fraction_half"].n_inliers >= 60 > refs["fraction_0"].n_inliers
    assert not refs["fraction_1"].found and refs["fraction_1"].n_valid > 0
    assert not refs["iterations_0"].found and len(refs["iterations_0"].counts) == 0 and len(refs["iterations_1"].counts) == 1
    assert refs["seed_0"].best_hypothesis != refs["seed_2_63"].best_hypothesis
    r = refs["past_a_batch"]
    assert r.found and len(r.counts) == C.MAX_BATCH + 1 and C.batch_cap(120) == C.MAX_BATCH
    assert refs["nonfinite_records"].found and refs["nonfinite_records"].n_inliers == 116
    assert refs["default_range"].n_inliers == 40
    # the scoring cases: the transforms spread from most records to none, the seams of the tree are there
    src, tgt, Ts, rng = C.SCORE_CASES["source_300"]
    counts, sums = R.score_transforms(Ts, src, tgt, rng)
    assert counts[1] > 200 and (counts[[0, 7, 8, 9, 10, 11]] == 0).all() and len(set(counts[1:7].tolist())) > 3
    assert len(C.SCORE_CASES["hypotheses_past_a_batch"][2]) == C.batch_cap(129) + 1
    line = C.SCORE_CASES["target_sliver"][1]
    assert np.ptp(line[:, 0]) > 1000 * max(np.ptp(line[:, 1]), np.ptp(line[:, 2]))
    for name, far in (("range_square_inf", 300), ("range_above_box", 0)):                # the two transforms that throw the source 2^20 m away
        src, tgt, Ts, rng = C.SCORE_CASES[name]
        assert (R.score_transforms(Ts, src, tgt, rng)[0][[7, 8]] == far).all()


def test_end_to_end_case_reaches_every_record(api):
    """the seed of prerej_cases.end_to_end is one for which the reference finds every source record an inlier"""
    src, tgt, nbr, prm = C.end_to_end()
    true_of = C.pair(400, 12)[2]
    held = (nbr == true_of[:, None]).any(axis=1).mean()
    assert 0.32 < held < 0.49 and nbr.shape == (400, 5)            # 400 draws at 0.4 (sd 0.025), and 5 / 400 by chance in the other rows: 3 sd either way
    r = R.prerejective(api, src, tgt, nbr, **prm)
    err = np.linalg.norm(r.transform.astype(np.float64) - C.TURN)
    print("end to end: winner %d, %d valid, |T - truth|_F = %.3g" % (r.best_hypothesis, r.n_valid, err))
    assert r.found and r.n_inliers == 400 and tuple(true_of[list(r.sample)]) == r.match


def test_plan_rule_owns_every_pair_once():
    """csrc/prerej_plan.hpp through tests/cpp/prerej_plan_rule.cpp, compiled with the sanitizers: the constants the cases mirror, the
    plan against its Python twin, every (tile, hypothesis) owned by exactly one workgroup, the workgroup count bounded, the batches
    and their cap."""
    at_cap = C.PARTIAL_BYTES // (C.MAX_BATCH * C.PARTIAL_STRIDE) * C.TILE           # the most records whose batch is still MAX_BATCH
    ns = (1, 127, 128, 129, 300, at_cap, at_cap + 1, (1 << 31) - 17)
    Hs = (1, C.CHUNK - 1, C.CHUNK, C.CHUNK + 1, C.MAX_BATCH, C.MAX_BATCH + 1, 1 << 20)
    sizes = [(n, H) for n in ns for H in Hs]
    cover = [(n, H) for n, H in sizes if -(-n // C.TILE) * H <= 1 << 22]
    batches = [(n, t) for n in ns for t in (0, 1, C.MAX_BATCH, C.MAX_BATCH + 1, 50000)]
    lines = ["plan %d %d" % s for s in sizes] + ["cover %d %d" % s for s in cover] + ["batches %d %d" % b for b in batches]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "prerej_plan_rule")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                            os.path.join(ROOT, "tests", "cpp", "prerej_plan_rule.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stdout[-3000:]
    out = r.stdout.strip().splitlines()
    assert out[0].split() == ["constants"] + [str(v) for v in (C.BLOCK, C.TILE, C.CHUNK, C.MAX_GROUPS, C.MAX_BATCH, C.ROUND, C.PARTIAL_BYTES, C.PARTIAL_STRIDE)]
    assert C.TILE == R.GROUP == 2 * R.WAVE and C.ROUND % C.MAX_BATCH == 0 and len(out) == 1 + len(lines)
    covered = grown = 0
    for line, want in zip(out[1:], lines):
        v = line.split()
        assert v[:len(want.split())] == want.split()
        if v[0] == "plan":
            n, H, tiles, chunks, per, slices = (int(x) for x in v[1:])
            assert (tiles, chunks, per, slices) == C.plan(n, H)
            assert tiles == -(-n // C.TILE) and chunks == -(-H // C.CHUNK) and 1 <= per <= chunks
            assert (slices - 1) * per < chunks <= slices * per                     # the slices tile the chunks, none is empty
            assert tiles * slices <= C.MAX_GROUPS + tiles < 2 ** 31                # bounded: one launch dimension holds the grid
            assert per == 1 or tiles * slices > C.MAX_GROUPS // 2                  # a slice grows only to keep that bound
            grown += per > 1
        elif v[0] == "cover":
            n, H, groups, bad = (int(x) for x in v[1:])
            tiles, chunks, per, slices = C.plan(n, H)
            assert groups == tiles * slices and bad == 0, line
            covered += 1
        else:
            n, total, cap = (int(x) for x in v[1:4])
            runs = [tuple(int(x) for x in w.split("x")) for w in v[4:]]
            assert cap == C.batch_cap(n) and 1 <= cap <= C.MAX_BATCH
            assert cap == C.MAX_BATCH or cap * -(-n // C.TILE) * C.PARTIAL_STRIDE <= C.PARTIAL_BYTES or cap == 1   # the partials stay under the stated size
            assert sum(b * t for b, t in runs) == total and all(b <= cap for b, t in runs)
            assert all(b == cap for b, t in runs[:-1]) and len(runs) <= 2             # whole batches, then the rest
    assert covered >= 30 and grown >= 3
    assert C.batch_cap(at_cap) == C.MAX_BATCH and C.batch_cap(at_cap + 1) == C.MAX_BATCH - 1 and C.batch_cap((1 << 31) - 17) == 1
