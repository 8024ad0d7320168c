"""The plane-segmentation contract without a GPU: the reference of tests/plane_seg_ref.py against a brute-force loop and against
the scenes' known planes; the host-only rules of csrc/plane_seg_plan.hpp -- the cut into workgroups, the batches and the stopping
rule with its skip counter -- through their stand-alone program; rsreg_plane_from_sums against numpy.linalg.eigh; the refusals that
need no device; and what every case of tests/plane_seg_cases.py is FOR, asserted on the reference, so that the GPU tests compare
bits on cases that reach the branches they name.
"""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import plane_seg_cases as K
import plane_seg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api(rs):
    from rsreg_amd import api, lib
    lib.build()
    return api


@pytest.fixture(scope="module")
def refs(api):
    out = {}

    def get(name):
        if name not in out:
            make, prm = K.SEGMENT_CASES[name]
            xyz = make()
            out[name] = (R.segment(api, xyz, **prm), xyz, prm)
        return out[name]
    return get


def _angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = abs(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))
    return math.acos(min(c, 1.0)) if c < 1.0 - 1e-9 else float(np.linalg.norm(np.cross(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b)))


def test_counts_equal_a_brute_force_loop():
    """R.count (vectorised) against a loop over records written apart from it: one float32 operation a line, abs() and the strict
    compare in double"""
    xyz, models = K.count_cloud(300), K.count_models(40)
    thr = 0.05
    want = np.zeros(len(models), np.uint32)
    with np.errstate(all="ignore"):
        for h, (a, b, c, d) in enumerate(models):
            for x, y, z in xyz:
                if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
                    continue
                s = np.float32(a * x)
                s = np.float32(s + np.float32(b * y))
                s = np.float32(s + np.float32(c * z))
                s = np.float32(s + d)
                want[h] += bool(float(abs(s)) < thr)
    got = R.count(models, xyz, thr)
    assert (got == want).all()
    assert got[1] == np.isfinite(xyz).all(axis=1).sum() and got[2] == 0          # the zero normal: |d| < thr admits every finite record, |d| > thr none
    assert (got[3:7] == 0).all() and got[11:].min() > 0                            # NaN and inf models admit nothing; the ordinary ones something
    assert (R.count(models, xyz, 0.0) == 0).all()                                  # threshold 0 admits nothing


def test_reference_finds_the_plane_of_scene_a_and_refinement_improves_it(refs):
    """The bound on the refined normal, from sigma and the extent.  In the frame of the true plane (normal along z, origin at the
    disc's centre) the least-squares tilt along one in-plane axis x is sum(x z) / sum(x x) over the m inliers.  The plane's own
    records lie on a disc of radius Rd = EXTENT / 2, so sum(x x) >= m_plane * Rd^2 / 4.  Three things move the tilt:
      noise: z ~ N(0, sigma^2) gives a standard error sigma / sqrt(sum(x x)); six of them bound it;
      truncation: the winner's band |dist| < T may cut one tail of the noise where the band's edge comes near, at worst half the
        distribution at the rim, which shifts the mean z there by at most E|z| = 0.8 sigma: a tilt of at most 0.8 sigma / Rd;
      clutter: a record of the cube inside the band has |z| <= T + Rd_c * (T / Rd) with lever |x| <= Rd_c = EXTENT * sqrt(3) / 2; the
        band holds a share 2 T * (EXTENT * sqrt(2))^2 / EXTENT^3 of the cube at most (its widest cross-section), three times the expected number
        bounds their count.
    The two in-plane axes add in quadrature."""
    xyz, on = K.scene_a(0.6, 0)
    n_plane, n_clutter = int(on.sum()), int((~on).sum())
    Rd, Rc, T, s = K.EXTENT / 2, K.EXTENT * math.sqrt(3) / 2, K.THRESHOLD, K.SIGMA
    sxx = n_plane * Rd * Rd / 4
    noise = 6 * s / math.sqrt(sxx)
    trunc = 0.8 * s / Rd
    in_band = 3 * n_clutter * 2 * T * (K.EXTENT * math.sqrt(2)) ** 2 / K.EXTENT ** 3
    clutter = in_band * Rc * (T + Rc * T / Rd) / sxx
    bound = math.sqrt(2) * (noise + trunc + clutter)
    assert 1e-3 < bound < T / Rd * 2                                               # tighter than what the band alone allows (2 T / Rd)
    for name in ("a60_s0", "a60_s1", "a60_s2"):
        r = refs(name)[0]
        assert r.found and r.refined and r.iterations < 50 and r.skipped == 0
        true_in = np.abs((xyz.astype(np.float64) - K.A_POINT) @ K.A_NORMAL) < T
        assert abs(r.n_inliers - int(true_in.sum())) <= 0.02 * n_plane and r.n_inliers > 0.97 * n_plane
        a_ref, a_unref = _angle(r.coeff[:3], K.A_NORMAL), _angle(r.unrefined[:3], K.A_NORMAL)
        assert a_ref < a_unref and a_ref <= bound, (name, a_ref, a_unref, bound)
        assert abs(float(np.linalg.norm(r.coeff[:3].astype(np.float64))) - 1.0) < 1e-6
        assert abs(float(r.coeff[:3].astype(np.float64) @ K.A_POINT + r.coeff[3])) < 3 * s      # the plane passes the disc's centre
        assert r.coeff[:3].astype(np.float64) @ r.unrefined[:3].astype(np.float64) > 0           # the sign rule


def test_cases_reach_the_branches_they_are_named_for(refs):
    """(the k-margin condition is asserted inside plane_seg_ref.Replay for every one of these cases)"""
    r = refs("a60_unrefined")[0]
    assert r.found and not r.refined and (r.coeff == r.unrefined).all() and (r.sums == 0).all()
    assert r.best_hypothesis == refs("a60_s0")[0].best_hypothesis and r.n_inliers == refs("a60_s0")[0].best
    r = refs("a30_exhausts_50")[0]
    assert r.found and r.iterations == 50 and r.ks[-1] > 50
    r = refs("a30_1000")[0]
    assert r.found and 50 < r.iterations < 1000 and r.iterations == max(math.ceil(r.ks[-1]), r.best_hypothesis + 1)
    xyz, label = K.scene_b(0)
    r = refs("b_plain")[0]
    assert r.found and r.skipped == 0 and abs(r.coeff[0]) > 0.99 and (label[r.inliers] == 0).mean() > 0.95 and r.n_inliers > 1100     # the wall
    for name in ("b_axis_z", "b_axis_z_s1"):
        r = refs(name)[0]
        assert r.found and abs(r.coeff[2]) > 0.99 and (label[r.inliers] == 1).mean() > 0.9 and r.n_inliers > 550                      # the floor
        assert 50 < r.iterations < 1000 and r.skipped > 10 * r.iterations and r.min_cs_margin > 1e-12
        assert r.iterations + r.skipped > K.FIRST_BATCH + 2 * K.FIRST_BATCH          # the replay crosses more than two batches
        assert abs(r.cos_eps - math.cos(K.EPS_10_DEG)) == 0
    r = refs("b_axis_skip_cap")[0]
    assert r.skipped == 500 and r.iterations < 50                                   # max_iterations 50: the skip cap ends it first
    for name in ("a60_shifted", "a60_scaled"):
        r = refs(name)[0]
        assert r.found and r.refined
    assert refs("a60_scaled")[0].n_inliers > 1100
    r = refs("collinear")[0]
    assert not r.found and r.iterations == 0 and r.skipped == 500 and (r.coeff == 0).all() and len(r.inliers) == 0
    r = refs("threshold_0")[0]
    assert not r.found and r.best == 0 and r.iterations == 50
    for name in ("n2", "n0"):
        r = refs(name)[0]
        assert not r.found and r.iterations == 0 and r.skipped == 0


def test_hypothesis_cases_reach_their_branches():
    for name, (make, prm) in K.HYPOTHESIS_CASES.items():
        xyz = make()
        models, samples, valid, cs = R.hypotheses(xyz, prm["seed"], 0, K.HYPOTHESES, prm.get("axis", (0, 0, 0)), prm.get("eps_angle", 0.0))
        tries = samples[:, 3]
        if name in ("collinear", "n2"):
            assert not valid.any() and (samples == -1).all() and np.isnan(models).all()
        if name == "n3":
            assert valid.sum() > 100 and (~valid).sum() >= 1 and (tries > 3).sum() > 20   # three draws from three records differ in 2 tries of 9
            assert len({tuple(m) for m in np.abs(models[valid])}) == 1              # the one plane, whatever the order of its records
        if name == "nans":
            assert valid.all() and (tries > 0).sum() > 50
            assert np.isfinite(xyz[samples[:, :3]]).all()
        if name == "duplicates":
            assert (tries > 0).sum() > 50 and valid.sum() > 100                     # (three of six points differ with probability 5/9)
        if name.startswith("axis"):
            cos_eps = math.cos(prm["eps_angle"])
            assert min(abs(c - cos_eps) for c in cs if c is not None) > 1e-12       # no hypothesis sits on the axis test's edge
            assert 3 < valid.sum() < K.HYPOTHESES - 3 and (tries >= 0).all()         # both outcomes; an axis failure keeps its sample
            assert np.isnan(models[~valid]).all() and np.isfinite(models[valid]).all()
        ok = models[valid].astype(np.float64)
        assert (np.abs(np.linalg.norm(ok[:, :3], axis=1) - 1.0) < 1e-6).all()
        for m, s in zip(models[valid][:10], samples[valid][:10]):                   # the three sample records lie on their plane
            assert (np.abs(xyz[s[:3]].astype(np.float64) @ m[:3].astype(np.float64) + float(m[3])) < 1e-5).all()


def test_threshold_records_sit_on_both_sides():
    inside_at = set()
    for t in (np.float32(0.01), 0.01, 0.0625, 1e-3):
        xyz = K.threshold_records(t)
        z = np.abs(xyz[:, 2])
        f = np.float32(t)
        assert sorted(set(z.tolist())) == [float(np.nextafter(f, np.float32(0))), float(f), float(np.nextafter(f, np.float32(np.inf)))]
        got = R.within([0, 0, 1, 0], xyz, float(t))[0]
        assert (got == (z.astype(np.float64) < float(t))).all() and got[:8].all() and not got[16:].any()
        inside_at.add(bool(got[8:16].all()))                                        # z == (float)t: inside iff the cast rounded DOWN
        assert got[8:16].all() or not got[8:16].any()
    assert inside_at == {True, False}


def test_tree_sum_is_the_contracts_tree():
    """against a literal walk of the tree for one sum, and against math.fsum within the depth's bound"""
    rng = np.random.default_rng(4)
    for n in (1, 63, 64, 65, 128, 129, 1000, 128 * 256 + 5):
        t = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n)
        groups = -(-n // 128)
        v = np.zeros(groups * 128)
        v[:n] = t
        part = []
        for g in range(groups):
            waves = []
            for w in range(2):
                lane = list(v[g * 128 + w * 64:g * 128 + w * 64 + 64])
                for bit in (32, 16, 8, 4, 2, 1):
                    lane = [lane[k] + lane[k + bit] for k in range(bit)]
                waves.append(lane[0])
            part.append(waves[0] + waves[1])
        strand = [0.0] * 256
        for g, p in enumerate(part):
            strand[g % 256] = strand[g % 256] + p
        tot = []
        for w in range(4):
            lane = strand[64 * w:64 * w + 64]
            for bit in (32, 16, 8, 4, 2, 1):
                lane = [lane[k] + lane[k + bit] for k in range(bit)]
            tot.append(lane[0])
        want = ((tot[0] + tot[1]) + tot[2]) + tot[3]
        got = float(R.tree_sum(t))
        assert got == want
        assert abs(got - math.fsum(t)) <= (16 + -(-groups // 256)) * 2.0 ** -53 * float(np.abs(t).sum())


def test_plan_rule_covers_every_cell_once_and_replays_the_stopping_rule():
    """csrc/plane_seg_plan.hpp through tests/cpp/plane_seg_plan_rule.cpp, compiled with the sanitizers: the constants the cases
    mirror, the plan against its Python twin, every (tile, chunk) cell owned by exactly one workgroup at the edges of every constant,
    the batches, and PlaneReplay -- the code the library runs -- on hand-written sequences and against the reference's replay."""
    edge = K.MAX_GROUPS * K.CHUNK                                                   # H at which one tile fills the group limit
    sizes = [(n, H) for n in (1, K.TILE - 1, K.TILE, K.TILE + 1, 3 * K.TILE + 5, 307200, 1 << 20, (1 << 31) - 17)
             for H in (1, K.CHUNK - 1, K.CHUNK, K.CHUNK + 1, 200, 4096, edge - 1, edge, edge + 1, 1 << 20)]
    cover = [(n, H) for n, H in sizes if -(-n // K.TILE) * -(-H // K.CHUNK) <= 1 << 20]
    max_its = (0, 1, 23, 24, 50, 70, 1000, 7936, 20000)
    # the hand-written sequences: (n, probability, max_iterations, [(valid, count)], want (best, winner, iterations, skipped))
    hand = [
        (100, 0.99, 50, [(0, 0), (1, 60), (1, 10)] + [(1, 5)] * 80, None),           # an invalid first hypothesis spends no iteration
        (100, 0.99, 5, [(0, 0)] * 60, (-1, -1, 0, 50)),                               # all invalid: ends at the skip cap, 10 * max_iterations
        (100, 0.99, 50, [(1, 40), (1, 40), (1, 39)] + [(1, 0)] * 80, None),          # a tie keeps the first
        (100, 0.99, 0, [(1, 90)] * 4, (-1, -1, 0, 0)),                                # max_iterations 0: nothing is consumed
        (100, 0.99, 3, [(1, 1), (0, 0), (1, 2), (0, 0), (1, 3), (1, 99)], (3, 4, 3, 2)),   # ends on max_iterations; the rest is not read
    ]
    rng = np.random.default_rng(8)
    rand = []
    for trial in range(60):
        n, max_it = int(rng.integers(3, 3000)), int(rng.integers(0, 60))
        L = 11 * max_it + 1
        valid = (rng.uniform(size=L) < float(rng.choice([0.05, 0.5, 1.0]))).astype(int)
        counts = rng.integers(0, max(2, n // int(rng.integers(1, 30))), L)
        rand.append((n, float(rng.choice([0.5, 0.99, 0.999999])), max_it, list(zip(valid.tolist(), counts.tolist())), None))
    replays = hand + rand
    lines = ["plan %d %d" % s for s in sizes] + ["cover %d %d" % s for s in cover] + ["batches %d" % m for m in max_its]
    lines += ["replay %d %r %d %d %s" % (n, p, m, len(seq), " ".join("%d %d" % vc for vc in seq)) for n, p, m, seq, _ in replays]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "plane_seg_plan_rule")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                            os.path.join(ROOT, "tests", "cpp", "plane_seg_plan_rule.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stdout[-3000:]
    out = r.stdout.strip().splitlines()
    assert out[0].split() == ["constants"] + [str(v) for v in (K.BLOCK, K.RECORDS_PER_LANE, K.TILE, K.CHUNK, K.MAX_GROUPS, K.FIRST_BATCH, K.MAX_BATCH, K.TRIES)]
    assert R.TRIES == K.TRIES and len(out) == 1 + len(lines)
    grown, it_replay = 0, iter(replays)
    for line, asked in zip(out[1:], lines):
        v = line.split()
        if v[0] == "plan":
            n, H, tiles, chunks, per, slices = (int(x) for x in v[1:])
            assert (tiles, chunks, per, slices) == K.plan(n, H) and "plan %d %d" % (n, H) == asked
            assert tiles == -(-n // K.TILE) and chunks == -(-H // K.CHUNK) and 1 <= per <= chunks
            assert (slices - 1) * per < chunks <= slices * per                      # the slices tile the chunks, none is empty
            assert tiles * slices <= K.MAX_GROUPS + tiles < 2 ** 31                 # bounded: one launch dimension holds the grid
            assert per == 1 or tiles * slices > K.MAX_GROUPS // 2                   # a slice grows only to keep that bound
            grown += per > 1
        elif v[0] == "cover":
            n, H, groups, bad = (int(x) for x in v[1:])
            tiles, chunks, per, slices = K.plan(n, H)
            assert groups == tiles * slices and bad == 0, line
        elif v[0] == "batches":
            m, got, (count, total) = int(v[1]), [int(x) for x in v[2:v.index("...")]], (int(x) for x in v[-2:])
            want_b, done = [], 0
            while K.batch(done, m) and len(want_b) < 64:
                want_b.append(K.batch(done, m))
                done += want_b[-1]
            assert got == want_b and total == min(11 * m, 0x7ffffff0) and all(b <= K.MAX_BATCH for b in got)
            assert got[:5] == [256, 512, 1024, 2048, 4096][:len(got[:5])] or sum(got[:5]) == 11 * m
        else:
            n, p, m, seq, want = next(it_replay)
            best, winner, it, skipped, consumed, ran_out = (int(x) for x in v[1:])
            assert not ran_out and consumed == it + skipped <= len(seq)
            assert it <= m and skipped <= 10 * m and consumed < max(11 * m, 1)      # what the cap of 11 * max_iterations rests on
            if want is not None:
                assert (best, winner, it, skipped) == want, line
            valid, counts = [a for a, _ in seq], [c for _, c in seq]
            assert (best, winner, it, skipped) == R.replay(counts, valid, n, p, m), line
    assert grown >= 5 and K.plan(3, edge)[2] == 1 and K.plan(3, edge + 1)[2] == 2 and K.plan(K.TILE + 1, edge // 2 + 1)[2] == 2
    # the hand-written ones once more, on the reference, spelled out
    assert R.replay([0, 60, 10] + [5] * 80, [0, 1, 1] + [1] * 80, 100, 0.99, 50)[1:] == (1, math.ceil(math.log(0.01) / math.log(1 - 0.6 ** 3)), 1)
    assert R.replay([40, 40, 39] + [0] * 80, [1] * 83, 100, 0.99, 50)[:2] == (40, 0)


def test_plane_from_sums_against_eigh(api):
    """rsreg_plane_from_sums (cyclic Jacobi in double, rounded to float) against numpy.linalg.eigh on the same sums.  On cases whose
    smallest eigen-gap is at least 1e-3 of the trace the two normals are within 1e-6 rad: rounding a unit vector to float costs up
    to about 1e-7, ten times less; the double Jacobi's own error is below 1e-9 there."""
    rng = np.random.default_rng(21)
    checked = flipped = 0
    for trial in range(200):
        m = int(rng.integers(3, 400))
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        basis = np.linalg.qr(np.column_stack([nrm, rng.normal(size=(3, 2))]))[0]
        scale = 10.0 ** rng.uniform(-3, 3)
        pts = (rng.normal(size=(m, 3)) * np.array([rng.uniform(0.001, 0.3), rng.uniform(0.5, 1), rng.uniform(0.5, 1)])) @ basis.T * scale
        p0 = (rng.normal(size=3) * scale).astype(np.float32)
        P = (pts + p0).astype(np.float32)
        flags = rng.uniform(size=m) < 0.8
        flags[:3] = True
        sums = R.ten_sums(P, flags, p0)
        prior = np.append(basis[:, 0] * rng.choice([-1.0, 1.0]), 0.0).astype(np.float32)
        want = R.plane_from_sums_eigh(sums, p0, prior)
        got = api.plane_from_sums(sums, p0, prior)
        assert got is not None and want is not None and got.dtype == np.float32
        mean = sums[1:4] / sums[0]
        Cm = np.array([[sums[4], sums[5], sums[6]], [sums[5], sums[7], sums[8]], [sums[6], sums[8], sums[9]]]) / sums[0] - np.outer(mean, mean)
        w = np.linalg.eigvalsh(Cm)
        if w[1] - w[0] < 1e-3 * w.sum():
            continue
        checked += 1
        g = got[:3].astype(np.float64)
        assert np.linalg.norm(np.cross(g, want[0])) / np.linalg.norm(g) <= 1e-6, (trial, got, want)
        assert g @ prior[:3].astype(np.float64) >= 0 and g @ want[0] > 0           # the sign rule: on the prior's side
        flipped += bool(prior[:3].astype(np.float64) @ basis[:, 0] < 0)
        assert abs(float(got[3]) - want[1]) <= 1e-6 * (abs(want[1]) + float(np.linalg.norm(p0.astype(np.float64) + mean))) + 1e-30
    assert checked > 150 and 30 < flipped < checked - 30
    # an exact case: the plane z = 2 sampled on a lattice, relative to a record of it
    gx, gy = np.meshgrid(np.arange(5.0), np.arange(4.0))
    P = np.stack([gx.ravel(), gy.ravel(), np.full(20, 2.0)], axis=1).astype(np.float32)
    sums = R.ten_sums(P, np.ones(20, bool), P[7])
    assert (api.plane_from_sums(sums, P[7], [0, 0, 1, 0]) == np.array([0, 0, 1, -2], np.float32)).all()
    assert (api.plane_from_sums(sums, P[7], [0, 0, -1, 0]) == np.array([0, 0, -1, 2], np.float32)).all()
    # the fallbacks: fewer than three inliers, a covariance that is not finite -- refused, nothing written
    two = R.ten_sums(P, np.arange(20) < 2, P[0])
    assert two[0] == 2 and api.plane_from_sums(two, P[0], [0, 0, 1, 0]) is None
    for bad in (np.nan, np.inf):
        s = sums.copy()
        s[5] = bad
        assert api.plane_from_sums(s, P[7], [0, 0, 1, 0]) is None
    s = sums.copy()
    s[4] = 1e308
    s[1] = 1e200                                                                    # mean * mean overflows: inf - inf
    assert api.plane_from_sums(s, P[7], [0, 0, 1, 0]) is None
    from rsreg_amd import lib as L
    out = np.full(4, 7.0, np.float32)
    assert L.lib().rsreg_plane_from_sums(two.ctypes.data, P[0].ctypes.data, np.zeros(4, np.float32).ctypes.data, out.ctypes.data) == L.RSREG_ERR_INVALID_ARG
    assert (out == 7.0).all()


def test_host_side_refusals_and_defaults(api):
    from rsreg_amd import lib as L
    h = L.lib()
    p = api.plane_params()
    assert (p.distance_threshold, p.max_iterations, p.probability, p.optimize_coefficients, tuple(p.axis), p.eps_angle, p.seed) == \
        (0.0, 50, 0.99, 1, (0.0, 0.0, 0.0), 0.0, 0)
    assert C.sizeof(L.PlaneParams) == 64 and C.sizeof(L.PlaneResult) == 64 + 8 * L.NUM_PLANE_SEG_SUMS and L.NUM_PLANE_SEG_SUMS == R.NUM_SUMS
    assert L.PlaneResult.n_inliers.offset == 32 and L.PlaneResult.cos_eps.offset == 40 and L.PlaneResult.unrefined.offset == 48
    with pytest.raises(TypeError):
        api.plane_params(inlier_threshold=1.0)
    assert h.rsreg_version() == 4
    buf = np.zeros(16, np.float64)
    z = C.c_size_t(0)
    for a in (None, buf.ctypes.data):                                               # any NULL argument of the host-only step
        for b in (None, buf.ctypes.data):
            for c in (None, buf.ctypes.data):
                for d in (None, buf.ctypes.data):
                    if None in (a, b, c, d):
                        assert h.rsreg_plane_from_sums(a, b, c, d) == L.RSREG_ERR_INVALID_ARG
    # without a context or a cloud every device entry point refuses before it touches a device
    assert h.rsreg_cloud_plane_count(None, None, buf.ctypes.data, 1, 0.1, buf.ctypes.data) == L.RSREG_ERR_INVALID_ARG
    assert h.rsreg_cloud_plane_hypotheses(None, None, C.byref(p), 0, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data) == L.RSREG_ERR_INVALID_ARG
    assert h.rsreg_cloud_plane_segment(None, None, C.byref(p), buf.ctypes.data, buf.ctypes.data, 1, C.byref(z), None) == L.RSREG_ERR_INVALID_ARG
    assert h.rsreg_cloud_plane_filter(None, None, buf.ctypes.data, 0.1, 0, 0, None, None) == L.RSREG_ERR_INVALID_ARG
    assert h.rsreg_cloud_extract_indices(None, None, buf.ctypes.data, 1, 0, None, None) == L.RSREG_ERR_INVALID_ARG
    h.rsreg_plane_params_default(None)                                              # a NULL struct is ignored
    seg = api.SACSegmentation()
    with pytest.raises(L.RsregError):
        seg.setModelType(5)                                                         # SACMODEL_CYLINDER
    with pytest.raises(L.RsregError):
        seg.setMethodType(1)                                                        # SAC_LMEDS
    with pytest.raises(L.RsregError):
        seg.segment()                                                               # no input cloud
    assert (seg.getMaxIterations(), seg.getProbability(), seg.getOptimizeCoefficients(), seg.getDistanceThreshold()) == (50, 0.99, True, 0.0)
    assert (api.SACMODEL_PLANE, api.SACMODEL_PERPENDICULAR_PLANE, api.SAC_RANSAC) == (0, 9, 0)
