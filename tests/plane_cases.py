"""Shared pieces of the point-to-plane GPU tests (tests/test_plane_icp_gpu.py, tests/test_plane_cpp_gpu.py): the three-wall
clouds, and one step-wise check -- begin -> search -> plane_sums -> update_plane -- against tests/plane_ref.py fed the
engine's own (index, d2).  `python plane_cases.py NAME` runs one check in a process of its own (the index kind is chosen per
process: tests/test_index_paths_gpu.py) and prints "plane case ok"."""
import os
import sys

import numpy as np

import filters_ref
import plane_ref

GATE = 0.05
F32_EPS = 2.0 ** -24


def cloud(xyz):
    from rsreg_amd import POINT_DTYPE, PointCloud
    pts = np.zeros(len(xyz), POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["w"] = 1.0
    return PointCloud(pts, width=len(xyz), height=1, is_dense=False)


def normal_cloud(api, nrm):
    rec = np.zeros(len(nrm), api.NORMAL_DTYPE)
    rec["normal_x"], rec["normal_y"], rec["normal_z"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    return api.NormalCloud(rec, len(nrm), 1, bool(np.isfinite(nrm).all()))


def three_walls(n, seed=3, extent=1.0):
    """n target points on the walls x = -1, y = 0.9, z = 2.2 of a room (a third each), with their inward normals."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-extent, extent, (n, 3))
    p[:, 2] += 1.2
    wall = np.arange(n) % 3
    value = np.array([-1.0, 0.9, 2.2])
    sign = np.array([1.0, -1.0, -1.0])
    nrm = np.zeros((n, 3))
    p[np.arange(n), wall] = value[wall]
    nrm[np.arange(n), wall] = sign[wall]
    return p.astype(np.float32), nrm.astype(np.float32)


def source_near(tgt, n, seed=4, x=(0.004, -0.006, 0.005, 0.006, -0.004, 0.008), noise=0.002):
    """n source points: target points (drawn with replacement), jittered, moved by the inverse of the small motion x."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(tgt), n)
    T = np.linalg.inv(plane_ref.euler_matrix(np.array(x)).astype(np.float64))
    p = tgt[pick].astype(np.float64) + rng.normal(0, noise, (n, 3))
    return (p @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def solve_tolerance(sums, T):
    """entries of the increment within cond(AtA) * 2^-50 (over the directions above the cut) plus one float rounding"""
    A, _ = plane_ref.system(sums)
    w = np.linalg.eigvalsh(A)
    w = w[w > plane_ref.rank_cut(sums)]
    cond = float(w[-1] / w[0]) if len(w) else 1.0
    return cond * 2.0 ** -50 + F32_EPS * np.maximum(np.abs(T), 1.0), cond


def stepwise_check(api, src, tgt, nrm, gate=GATE, guess=None, ctx=None, ctx2=None, set_target=None, label="", **params):
    """One iteration, step by step, on `ctx`; the point-to-point sums of the same search on `ctx2`.  Returns the 32 sums."""
    ctx = ctx or api.Context(0)
    ctx2 = ctx2 or api.Context(0)
    icp = api.IterativeClosestPointWithNormals(ctx)
    p2p = api.IterativeClosestPoint(ctx2)
    for o in (icp, p2p):
        o.setMaxCorrespondenceDistance(gate)
        for k, v in params.items():
            setattr(o.params, k, v)
        o.setInputSource(cloud(src))
    if set_target is not None:
        set_target(icp)
    else:
        icp.setInputTarget(cloud(tgt), normal_cloud(api, nrm))
    p2p.setInputTarget(cloud(tgt))
    icp.begin(guess)
    idx, d2 = icp.search()
    sums = icp.plane_sums()
    p2p.begin(guess)
    idx2, d22 = p2p.search()
    s17 = p2p.sums()
    assert (idx == idx2).all() and (d2 == d22).all()
    assert sums[0] == s17[0] and sums[1].tobytes() == s17[16].tobytes(), (label, sums[:2], s17[[0, 16]])
    # the reference over the pairs the engine reports, at the positions the engine searched from
    cur = filters_ref.xyz(cloud(src))
    fin = np.isfinite(cur).all(axis=1)
    if guess is not None:
        cur[fin] = filters_ref.transform(cur[fin], guess)
    k = np.flatnonzero(idx >= 0)
    assert fin[k].all() and (idx[k] < len(tgt)).all()
    assert not (d2[k].astype(np.float64) > gate * gate).any()
    assert (d2[k] == plane_ref.d2_f32(cur[k], tgt[idx[k]])).all()
    ref, mag, cnt = plane_ref.plane_sums(cur[k], tgt[idx[k]], nrm[idx[k]], np.ones(len(k)), d2[k])
    bound = plane_ref.sums_bound(mag, cnt)
    err = np.abs(sums - ref)
    print("%s: %d pairs, %d in the system, worst error / bound %.3g" % (label, len(k), int(cnt[2]), float(np.max(err / np.maximum(bound, 1e-300)))))
    assert (err <= bound).all(), (label, np.flatnonzero(err > bound), err, bound)
    assert sums[0] == len(k) and sums[2] == cnt[2] and sums[31] == 0.0
    T_inc, done = icp.update_plane(sums)
    if sums[0] < 3:
        res = icp.end()
        assert done and api.CONV_STATES[res.state] == "NO_CORRESPONDENCES"
        return sums
    T_ref, rank = plane_ref.plane_solve(sums)
    tol, cond = solve_tolerance(sums, T_ref)
    print("%s: rank %d, cond %.3g" % (label, rank, cond))
    assert (np.abs(T_inc.astype(np.float64) - T_ref) <= tol).all(), (label, T_inc, T_ref)
    assert (api.plane_solve_from_sums(sums) == T_inc).all()
    res = icp.end()
    assert res.iterations == 1 and res.n_correspondences == len(k)
    last = np.array(res.sums_last)
    assert last[0] == sums[0] and last[16] == sums[1] and not last[1:16].any()
    assert (icp.plane_sums_last() == sums).all()
    return sums


def main(name):
    import rsreg_amd  # noqa: F401
    from rsreg_amd import api
    if name == "walls_index_kind":
        tgt, nrm = three_walls(2000)
        src = source_near(tgt, 1000)
        want = int(os.environ["PLANE_CASE_INDEX_KIND"])
        kinds = []

        def set_target(icp):
            icp.setInputTarget(cloud(tgt), normal_cloud(api, nrm))
            kinds.append(icp)
        sums = stepwise_check(api, src, tgt, nrm, set_target=set_target, label=name)
        # (the context is the last alignment's: its target index is the one the search ran over)
        icp = kinds[0]
        assert icp.grid_info().index_kind == want, (icp.grid_info().index_kind, want)
        print("sums", sums.tobytes().hex())
    else:
        raise SystemExit("unknown case " + name)
    print("plane case ok")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main(sys.argv[1])
