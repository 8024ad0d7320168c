"""Inputs and the lock-step loop shared by the rejector chain's GPU tests (tests/test_rejectors_gpu.py) and by the child process
that runs the same loop with RSREG_SORT_SMALL=1 (`python rejector_cases.py`): two contexts on the same pair, A without a chain,
B with it, both updated with B's sums so that their sources stay bit-equal; B's pairs, counts and sums against
tests/rejectors_ref.py over A's pairs, iteration by iteration, without a tolerance on the pairs."""
import functools
import json
import os
import sys

import numpy as np

import filters_ref as R
import rejectors_ref as J
from test_filter_ties import H, lattice_pair

GATE = 0.01
ITERATIONS = 4
# the chains of the whole-alignment cases, by name: (kind, value)
CHAINS = {
    "median": [(1, 1.0)],
    "one-to-one": [(2, 0.0)],
    "normal": [(3, 0.7)],
    "trimmed": [(4, 0.6)],
    "median,one-to-one": [(1, 1.0), (2, 0.0)],
    "one-to-one,median": [(2, 0.0), (1, 1.5)],
    "normal,one-to-one,median": [(3, 0.5), (2, 0.0), (1, 1.0)],
    "trimmed,one-to-one": [(4, 0.7), (2, 0.0)],
}


def cloud(xyz):
    from rsreg_amd import POINT_DTYPE, PointCloud
    pts = np.zeros(len(xyz), POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["w"] = 1.0
    return PointCloud(pts, width=len(xyz), height=1, is_dense=False)


def lattice_guess():
    """A translation by whole lattice steps: not the identity, and the first search still meets blocks of bit-equal d2."""
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (2 * H, -H, H)
    return T


@functools.lru_cache(maxsize=None)
def frames():
    """(source, target, guess) of the 50 k "parity" pair as (n, 3) float32."""
    from rsreg_amd import synth
    guess = synth.small_transform(0.05, (0.0004, -0.0002, 0.0003)).astype(np.float32)
    return R.xyz(synth.render_frame(1, "50k", "parity")), R.xyz(synth.render_frame(0, "50k", "parity")), guess


@functools.lru_cache(maxsize=None)
def big_lattice():
    """70 001 records (above the 65 536 of the plain path) with the lattice's copies and a few more, scattered."""
    src, tgt, a_pos, b_pos = lattice_pair(70001)
    src = src.copy()
    rng = np.random.default_rng(4)
    src[rng.choice(len(src), 40, replace=False)] = src[a_pos[0]]
    return src, tgt


def pair(name):
    if name == "lattice":
        s, t = lattice_pair(3000)[:2]
        return s, t, lattice_guess()
    if name == "big-lattice":
        s, t = big_lattice()
        return s, t, lattice_guess()
    return frames()


_NORMALS = {}


def normals_of(api, ctx, name, xyz):
    """rsreg_cloud_normals (k = 10) of a cloud, on the host: (n, 3) float32, NaN rows for non-finite records."""
    if name not in _NORMALS:
        dc = api.DeviceCloud(cloud(xyz), ctx)
        _NORMALS[name] = np.ascontiguousarray(dc.normals(10)[:, :3])
        dc.close()
    return _NORMALS[name]


def make_rejectors(api, chain):
    cls = {1: api.CorrespondenceRejectorMedianDistance, 3: api.CorrespondenceRejectorSurfaceNormal, 4: api.CorrespondenceRejectorTrimmed}
    return [api.CorrespondenceRejectorOneToOne() if k == 2 else cls[k](v) for k, v in chain]


def make_icp(api, ctx, src, tgt, chain=(), reciprocal=0, ratio=0.0, plane=False, src_n=None, tgt_n=None, pipeline=0, iterations=ITERATIONS,
             gate=GATE):
    icp = (api.IterativeClosestPointWithNormals if plane else api.IterativeClosestPoint)(ctx)
    est = icp.params.estimation
    icp.params = api.icp_params(max_iterations=iterations, criteria_mode=1, max_correspondence_distance=gate, pipeline_mode=pipeline)
    icp.params.estimation = est
    icp.setUseReciprocalCorrespondences(reciprocal)
    icp.setTrimmedRejectorOverlapRatio(ratio)
    for r in make_rejectors(api, chain):
        icp.addCorrespondenceRejector(r)
    icp.setInputSource(cloud(src))
    if plane:
        icp.setInputTarget(cloud(tgt), tgt_n)
    else:
        icp.setInputTarget(cloud(tgt))
    if any(k == 3 for k, _ in chain):
        icp.setInputSourceNormals(src_n)
        icp.setInputTargetNormals(tgt_n)
    return icp


def lockstep(api, ctx_a, ctx_b, src, tgt, guess, chain, reciprocal=0, ratio=0.0, plane=False, src_n=None, tgt_n=None, iterations=ITERATIONS,
             expect_merged=None):
    """The loop of the module's docstring; returns what it saw per iteration: (pairs in play, pairs kept, stats, A's index and d2,
    the kept index)."""
    a = make_icp(api, ctx_a, src, tgt, (), reciprocal, ratio, plane, src_n, tgt_n, iterations=iterations)
    b = make_icp(api, ctx_b, src, tgt, chain, reciprocal, ratio, plane, src_n, tgt_n, iterations=iterations)
    a.begin(guess)
    b.begin(guess)
    if expect_merged is not None:
        assert (b.grid_info().n_source_distinct < len(src)) == expect_merged, (b.grid_info().n_source_distinct, len(src))
    cur = R.transform(src, guess)
    identity = guess is None or np.array_equal(np.asarray(guess, np.float32), np.eye(4, dtype=np.float32))
    cur_n = None if src_n is None else (src_n.copy() if identity else J.rotate_normals(src_n, guess))
    seen = []
    for it in range(iterations):
        ia, da = a.search()
        ib, db = b.search()
        stats = b.rejector_stats()
        want, wstats = J.apply_chain(ia, da, chain, cur_n, tgt_n)
        np.testing.assert_array_equal(ib, want, err_msg="iteration %d" % it)
        np.testing.assert_array_equal(db[ia >= 0], da[ia >= 0])
        assert [(s[0], s[1]) for s in stats] == [(s[0], s[1]) for s in wstats], (it, stats, wstats)
        assert [np.float32(s[2]) for s in stats] == [np.float32(s[2]) for s in wstats], (it, stats, wstats)
        kept = int((want >= 0).sum())
        seen.append((int((ia >= 0).sum()), kept, stats, ia, da, want))
        if plane:
            sums = b.plane_sums()
            assert sums[0] == kept
            np.testing.assert_allclose(sums[1], da[want >= 0].astype(np.float64).sum(), rtol=1e-11, atol=1e-11)
            if kept < 3:
                break
            t_inc, done = b.update_plane(sums)
            a.update_plane(sums)
        else:
            sums = b.sums()
            assert sums[0] == kept
            np.testing.assert_allclose(sums, R.sums(cur, tgt, want, da), rtol=1e-11, atol=1e-11)
            if kept < 3:
                break
            t_inc, done = b.update(sums)
            a.update(sums)
        cur = R.transform(cur, t_inc)
        if cur_n is not None:
            cur_n = J.rotate_normals(cur_n, t_inc)
    a.end()
    b.end()
    return seen


def stepwise(api, ctx, src, tgt, guess, chain, src_n=None, tgt_n=None, iterations=ITERATIONS):
    """A whole alignment through begin / search / sums / update / end: (iterations, correspondences, transform)."""
    icp = make_icp(api, ctx, src, tgt, chain, src_n=src_n, tgt_n=tgt_n, iterations=iterations)
    icp.begin(guess)
    done = False
    while not done:
        icp.search(want_output=False)
        _, done = icp.update(icp.sums())
    res = icp.end()
    return res.iterations, res.n_correspondences, icp.getFinalTransformation()


def run_lockstep_cases(api, merged, names=("lattice", "frames")):
    """Every chain of CHAINS over the named pairs, and one case with the two filters in front; `merged`: the source path expected."""
    out = {}
    for name in names:
        src, tgt, guess = pair(name)
        ctx_a, ctx_b = api.Context(0), api.Context(0)
        src_n, tgt_n = normals_of(api, ctx_a, name + "-src", src), normals_of(api, ctx_a, name + "-tgt", tgt)
        for cname, chain in CHAINS.items():
            seen = lockstep(api, ctx_a, ctx_b, src, tgt, guess, chain, src_n=src_n, tgt_n=tgt_n, expect_merged=merged)
            out["%s/%s" % (name, cname)] = [(s[0], s[1]) for s in seen]
        seen = lockstep(api, ctx_a, ctx_b, src, tgt, guess, CHAINS["one-to-one,median"], reciprocal=1, ratio=0.8, expect_merged=merged)
        out["%s/filters+one-to-one,median" % name] = [(s[0], s[1]) for s in seen]
        ctx_a.close()
        ctx_b.close()
    return out


@functools.lru_cache(maxsize=None)
def outlier_pair():
    """(source, target, ground truth, guess) of the 50 k "bench" pair with every fifth valid source record pushed 2 to 4 cm along
    its viewing ray, towards or away from the camera: flying pixels off the surface, inside a 5 cm gate.  The guess is a coarse
    alignment's result, the ground truth off by 0.2 degrees and 2.7 mm (|guess - truth|_F = 0.0056): the rejectors steady a
    REFINEMENT.  (From the identity, 1.5 degrees and 1.6 cm away, point-to-point ICP over this room's planes creeps, and keeping the
    closer half of the pairs makes it creep slower: after 30 iterations the numpy loop is 0.0107 off without a chain and 0.0507 --
    further than it began, 0.0404 -- with [ONE_TO_ONE, MEDIAN_DISTANCE].)"""
    from rsreg_amd import synth
    src = R.xyz(synth.render_frame(1, "50k", "bench")).copy()
    tgt = R.xyz(synth.render_frame(0, "50k", "bench"))
    rng = np.random.default_rng(77)
    valid = np.nonzero((src != 0).any(1))[0]
    hit = valid[rng.random(len(valid)) < 0.2]
    rng_len = np.linalg.norm(src[hit].astype(np.float64), axis=1)
    push = rng.uniform(0.02, 0.04, len(hit)) * rng.choice([-1.0, 1.0], len(hit))
    src[hit] = (src[hit].astype(np.float64) * (1.0 + push / rng_len)[:, None]).astype(np.float32)
    truth = synth.ground_truth(1, 0, "bench")
    return src, tgt, truth, (truth @ synth.small_transform(0.2, (0.002, -0.001, 0.0015))).astype(np.float32)


OUTLIER_GATE, OUTLIER_ITERATIONS, OUTLIER_CHAIN = 0.05, 30, [(2, 0.0), (1, 1.0)]


def edge_inputs():
    """The lattice with axis-aligned normals: target normals +z (two NaN ones among them); source normals +z, +y, 0.5 z and NaN in
    turn, so the float dot product is exactly 1, 0, 0.5 or NaN -- the 24 interleaved copies of A and B take all four."""
    src, tgt, a_pos, b_pos = lattice_pair(3000)
    tgt_n = np.zeros((len(tgt), 3), np.float32)
    tgt_n[:, 2] = 1.0
    matched = R.search(src, tgt, GATE)[0]
    k = np.arange(len(src)) % 4
    both = np.sort(np.concatenate([a_pos, b_pos]))
    k[both] = np.arange(len(both)) % 4                     # A, B, A, B, ... in index order: each point's copies get +z and 0.5 z, or +y and NaN
    k[both[:2]] = 0
    tgt_n[np.unique(matched[(matched >= 0) & (k == 0)])[:2], 0] = np.nan   # two targets that +z source records are matched to
    src_n = np.zeros((len(src), 3), np.float32)
    src_n[k == 0, 2] = 1.0
    src_n[k == 1, 1] = 1.0
    src_n[k == 2, 2] = 0.5
    src_n[k == 3] = np.nan
    return src, tgt, a_pos, b_pos, src_n, tgt_n, k


def run_edge_cases(api, merged):
    """Ties and edges on the first search of the lattice (identity guess: every block of bit-equal d2 intact); asserts what each case
    is about on the reference's side -- the engine is held to the reference by lockstep()."""
    src, tgt, a_pos, b_pos, src_n, tgt_n, k = edge_inputs()
    ctx_a, ctx_b = api.Context(0), api.Context(0)
    out = {}

    def first(chain, s=src, t=tgt, sn=src_n, tn=tgt_n, expect=merged):
        return lockstep(api, ctx_a, ctx_b, s, t, None, chain, src_n=sn, tgt_n=tn, iterations=1, expect_merged=expect)[0]

    # the median inside a block of equal d2, factor 1: everything at the bound stays
    m, kept, stats, ia, da, want = first([(1, 1.0)])
    med = np.float32(stats[0][2])
    play = np.sort(da[ia >= 0])
    assert play[m // 2] == med and play[m // 2 - 1] == med and play[min(m // 2 + 1, m - 1)] == med, "the median is not inside a tied block"
    assert kept == int((play <= med).sum()) > m // 2 + 1
    out["median-in-tie"] = (m, kept)
    # factor 0 with pairs at d2 = 0: those alone stay
    m, kept, stats, ia, da, want = first([(1, 0.0)])
    assert kept == int(((ia >= 0) & (da == 0)).sum()) > 0 and stats[0][2] > 0
    out["factor-0"] = (m, kept)
    # one-to-one: the 12 copies of A share a target at equal d2 -- at most the lowest index stays; the same for B
    m, kept, stats, ia, da, want = first([(2, 0.0)])
    assert len(set(ia[a_pos])) == 1 and len(set(da[a_pos])) == 1 and ia[a_pos[0]] >= 0
    assert (want[a_pos[1:]] == -1).all() and (want[b_pos[1:]] == -1).all()
    rivals = (ia == ia[a_pos[0]]) & ((da < da[a_pos[0]]) | ((da == da[a_pos[0]]) & (np.arange(len(ia)) < a_pos[0])))
    assert (want[a_pos[0]] >= 0) == (not rivals.any())
    assert kept == len(set(ia[ia >= 0]))
    out["one-to-one-copies"] = (m, kept)
    # a TRIMMED entry behind ONE_TO_ONE
    m, kept, stats, ia, da, want = first([(2, 0.0), (4, 0.6)])
    assert kept == R.trim_keep(0.6, stats[0][1]) < stats[0][1]
    out["one-to-one,trimmed"] = (m, kept)
    # the normal test at a threshold equal to a score that occurs (0.5): strict, so 0.5 goes; NaN on either side goes; the copies of
    # A and B keep exactly those whose own normal is +z
    m, kept, stats, ia, da, want = first([(3, 0.5)])
    ok_t = ~np.isnan(tgt_n[np.maximum(ia, 0)]).any(1)
    np.testing.assert_array_equal(want >= 0, (ia >= 0) & (k == 0) & ok_t)
    both = np.concatenate([a_pos, b_pos])
    assert 0 < (want[both] >= 0).sum() < len(both) and ((ia >= 0) & (k == 2)).any() and ((ia >= 0) & ~ok_t).any()
    out["normal-strict"] = (m, kept)
    m, kept, stats, ia, da, want = first([(3, 0.5), (2, 0.0), (1, 1.0)])
    out["normal,one-to-one,median"] = (m, kept)
    # m = 0, 1 and 2: a handful of records, of which 0, 1 or 2 lie within the gate
    far = np.full((5, 3), 50.0, np.float32)
    far[4] = np.nan
    for n_in in (0, 1, 2):
        s = far.copy()
        s[:n_in] = tgt[:n_in] + np.float32(H)
        m, kept, stats, ia, da, want = first([(1, 1.0), (2, 0.0)], s=s, sn=None, tn=None, expect=False if not merged else None)
        assert m == n_in and kept == n_in and stats[0][2] == (0.0 if n_in == 0 else float(np.float32(3 * H * H)))
        out["m-%d" % n_in] = (m, kept)
    # a target of one record: one-to-one leaves one pair
    one = tgt[:1].copy()
    near = (one + np.array([[H, 0, 0], [0, H, 0], [2 * H, 0, 0], [0, -H, 0]], np.float32)).astype(np.float32)
    m, kept, stats, ia, da, want = first([(2, 0.0), (1, 1.0)], s=near, t=one, sn=None, tn=None, expect=False if not merged else None)
    assert m == 4 and kept == 1 and want[0] == 0
    out["one-target"] = (m, kept)
    ctx_a.close()
    ctx_b.close()
    return out


if __name__ == "__main__":   # the child of test_rejectors_gpu.py: the environment (RSREG_SORT_SMALL) is the parent's choice
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from rsreg_amd import api as _api
    _merged = os.environ.get("RSREG_SORT_SMALL") == "1"
    print("RESULT " + json.dumps({"lockstep": run_lockstep_cases(_api, merged=_merged), "edges": run_edge_cases(_api, merged=_merged)}))
