"""Shared pieces of the GICP tests (tests/test_gicp_cpu.py, tests/test_gicp_gpu.py): the whole-alignment cases with their
reference covariances and reference alignment (computed once per process), and one step-wise check on the GPU -- begin -> search
-> gicp_sums(X) -- against tests/gicp_ref.py fed the engine's own (index, d2).  `python gicp_cases.py NAME` runs one check in a
process of its own (the index kind is chosen per process) and prints "gicp case ok"."""
import functools
import os
import sys

import numpy as np

import filters_ref
import gicp_ref
import plane_ref
from plane_cases import cloud, source_near, three_walls

K, EPSILON = 20, 1e-3
TIGHT = dict(transformation_epsilon=1e-7, rotation_epsilon=1e-7, max_iterations=60)
# the increment the sums are also taken at: a few milliradians and millimetres, as an inner step is
X_TEST = gicp_ref.delta(np.array([0.003, -0.002, 0.004, 0.002, -0.003, 0.001]))

# name -> (target points, source points, seeds, the motion source_near undoes, gate)
_ALIGN = {
    "walls5k": dict(n_tgt=5000, n_src=5000, seed=(3, 4), x=(0.004, -0.006, 0.005, 0.006, -0.004, 0.008), gate=0.25),
    "walls50k": dict(n_tgt=50_000, n_src=50_000, seed=(5, 6), x=(0.01, 0.008, -0.012, -0.02, 0.015, 0.01), gate=0.25),
}
ALIGN_CASES = tuple(_ALIGN)
# |T - truth|_F the reference reaches at the fixed point (tight epsilons), measured once on the reference alone (2.56e-4 from 1.64e-2
# on walls5k, 4.78e-5 from 3.66e-2 on walls50k) and pinned with a factor of 2 for margin: the source carries 2 mm of noise, so the
# fixed point is the noisy clouds' optimum, not the truth.  tests/test_gicp_cpu.py asserts it on the reference, the GPU test on the engine.
TRUTH_MARGIN = {"walls5k": 2 * 2.56e-4, "walls50k": 2 * 4.78e-5}


class Case:
    """src, tgt (float32), cov_s, cov_t (float64 (n, 6), the reference's), truth (float64 4 x 4), prm (gicp_ref.Params)"""


@functools.lru_cache(maxsize=None)
def align_case(name):
    d = _ALIGN[name]
    c = Case()
    c.tgt, _ = three_walls(d["n_tgt"], seed=d["seed"][0])
    c.src = source_near(c.tgt, d["n_src"], seed=d["seed"][1], x=d["x"])
    c.truth = plane_ref.euler_matrix(np.array(d["x"])).astype(np.float64)
    c.cov_s = gicp_ref.covariances(c.src, K, EPSILON).cov
    c.cov_t = gicp_ref.covariances(c.tgt, K, EPSILON).cov
    c.prm = gicp_ref.Params(max_correspondence_distance=d["gate"], **TIGHT)
    return c


@functools.lru_cache(maxsize=None)
def align_reference(name):
    c = align_case(name)
    return gicp_ref.gicp(c.src, c.tgt, c.cov_s, c.cov_t, None, c.prm, truth=c.truth)


def plane_covariances(nrm, epsilon=EPSILON):
    """I - (1 - eps) n n^T of given unit normals (the three walls' own): covariances without a search."""
    return gicp_ref.regularised(np.asarray(nrm, np.float64), epsilon)


def make_gicp(api, ctx, src, tgt, cov_s, cov_t, gate, **params):
    g = api.GeneralizedIterativeClosestPoint(ctx)
    g.setMaxCorrespondenceDistance(gate)
    for k, v in params.items():
        setattr(g.gparams, k, v)
    g.setInputSource(src if hasattr(src, "points") or isinstance(src, api.DeviceCloud) else cloud(src))
    g.setInputTarget(tgt if hasattr(tgt, "points") or isinstance(tgt, api.DeviceCloud) else cloud(tgt))
    g.setSourceCovariances(cov_s)
    g.setTargetCovariances(cov_t)
    return g


def stepwise_check(api, src, tgt, cov_s, cov_t, gate=0.05, guess=None, ctx=None, ctx2=None, label=""):
    """One search and the sums at I and at X_TEST on `ctx`; the point-to-point sums of the same search on `ctx2`.  Returns the
    sums at I, at X_TEST, and the reference's pair masks (kept pairs, pairs in the system)."""
    ctx = ctx or api.Context(0)
    ctx2 = ctx2 or api.Context(0)
    g = make_gicp(api, ctx, src, tgt, cov_s, cov_t, gate)
    p2p = api.IterativeClosestPoint(ctx2)
    p2p.setMaxCorrespondenceDistance(gate)
    p2p.setInputSource(cloud(src))
    p2p.setInputTarget(cloud(tgt))
    g.begin(guess)
    idx, d2 = g.search()
    p2p.begin(guess)
    idx2, d22 = p2p.search()
    s17 = p2p.sums()
    p2p.end()
    assert (idx == idx2).all() and (d2 == d22).all()
    cur = np.ascontiguousarray(src, np.float32).copy()
    fin = np.isfinite(cur).all(axis=1)
    T = np.eye(4, dtype=np.float32) if guess is None else np.asarray(guess, np.float32)
    if guess is not None:
        cur[fin] = filters_ref.transform(cur[fin], guess)
    k = np.flatnonzero(idx >= 0)
    assert fin[k].all() and (idx[k] < len(tgt)).all()
    assert not (d2[k].astype(np.float64) > gate * gate).any()
    assert (d2[k] == plane_ref.d2_f32(cur[k], tgt[idx[k]])).all()
    M, ok = gicp_ref.mahalanobis(np.asarray(cov_s)[k], np.asarray(cov_t)[idx[k]], T[:3, :3].astype(np.float64))
    out = []
    for name, X in (("I", None), ("X", X_TEST)):
        sums = g.gicp_sums(X)
        assert sums[0] == s17[0] and sums[1].tobytes() == s17[16].tobytes(), (label, name, sums[:2], s17[[0, 16]])
        ref, mag, cnt = gicp_ref.gicp_sums(cur[k], tgt[idx[k]], M, ok, np.ones(len(k)), d2[k], X)
        bound = gicp_ref.sums_bound(mag, cnt)
        err = np.abs(sums - ref)
        print("%s at %s: %d pairs, %d in the system, worst error / bound %.3g" % (label, name, len(k), int(cnt[2]), float(np.max(err / np.maximum(bound, 1e-300)))))
        assert (err <= bound).all(), (label, name, np.flatnonzero(err > bound), err, bound)
        assert sums[0] == len(k) and sums[2] == cnt[2] and sums[31] == 0.0
        out.append(sums)
    # the host-only solve of the sums at I against the reference's (numpy.linalg.eigh in the place of the Jacobi)
    x, D, rank = api.gicp_step_from_sums(out[0])
    xr, Dr, rank_r = gicp_ref.step(out[0])
    if out[0][2] >= 6:
        A, _ = plane_ref.system(out[0])
        w = np.linalg.eigvalsh(A)
        w = w[w > plane_ref.rank_cut(out[0])]
        cond = float(w[-1] / w[0]) if len(w) else 1.0
        assert rank == rank_r and np.abs(x - xr).max() <= cond * 2.0 ** -50 * max(1.0, np.abs(xr).max()), (label, x, xr, cond)
        assert np.abs(D - Dr).max() <= cond * 2.0 ** -49 * max(1.0, np.abs(xr).max())
    done = g.update(None, out[0], 1)
    res = g.end()
    assert res.n_correspondences == len(k) and res.inner_evaluations == 1
    assert np.array(res.sums_last).tobytes() == out[0].tobytes()
    if len(k) < 4:
        assert done and api.CONV_STATES[res.state] == "NO_CORRESPONDENCES" and res.iterations == 0
    else:
        assert res.iterations == 1 and res.mse == out[0][1] / out[0][0]
    return out[0], out[1], k, ok, g


def engine_stepwise_align(api, g, guess=None):
    """The whole alignment driven from here through the step-wise calls: gicp_ref.minimise over the engine's sums and the engine's
    own host solve -- the loop rsreg_gicp_align runs inside the library, call for call."""
    prm = g.gparams

    def step_fn(S, scale):
        return api.gicp_step_from_sums(S, scale)
    g.begin(guess)
    done = False
    while not done:
        g.search(want_output=False)
        X, S, evals = gicp_ref.minimise(g.gicp_sums, prm, step_fn)
        done = g.update(X, S, evals)
    return g.end()


def main(name):
    import rsreg_amd  # noqa: F401
    from rsreg_amd import api
    if name == "walls_index_kind":
        tgt, nrm = three_walls(2000)
        src = source_near(tgt, 1000)
        cov_t = plane_covariances(nrm)
        cov_s = plane_covariances(nrm[np.random.default_rng(4).integers(0, len(tgt), 1000)])
        want = int(os.environ["GICP_CASE_INDEX_KIND"])
        s_i, s_x, _, _, g = stepwise_check(api, src, tgt, cov_s, cov_t, label=name)
        assert g.grid_info().index_kind == want, (g.grid_info().index_kind, want)
        print("sums", s_i.tobytes().hex(), s_x.tobytes().hex())
    else:
        raise SystemExit("unknown case " + name)
    print("gicp case ok")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main(sys.argv[1])
