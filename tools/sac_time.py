"""The whole feature-based pre-alignment on two rendered frames a known LARGE motion apart, with host wall times of its last
stage: VoxelGrid -> NormalEstimation(10) -> FPFHEstimation(10) -> reciprocal correspondences -> sac_correspondences (RANSAC over
the correspondences) -> ICP from that pose.  Per leaf one line: the first call and the best repeat of rsreg_cloud_sac_correspondences
and of rsreg_cloud_count_inliers on the SAME hypotheses; count_inliers as a share of its issue bound, n * H * 27 float operations
over 256 CUs x 128 lanes x 2.4 GHz (the denominator of tools/feature_match_time.py), once at the rejector's own size, where the call
around the kernel is most of the time, and once with the transforms repeated up to --count-hypotheses; a numpy scoring of the same
hypotheses in the same run; and the Frobenius distance of the pose from the ground truth after RANSAC, after ICP from it, and after ICP from the
identity.  Everything is reported, nothing asserted.

    python tools/sac_time.py [--frames 0,20] [--leaves 0.06,0.03] [--size N300] [--hypotheses 4096] [--count-hypotheses 262144] [--repeats 3] [--out profiles/sac_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rsreg_amd  # noqa: E402,F401
from rsreg_amd import api  # noqa: E402
from rsreg_amd import synth  # noqa: E402

PEAK_FLOPS = 256 * 128 * 2.4e9    # 256 CUs x 128 fp32 lanes x 2.4 GHz, one operation a lane a clock (no FMA: the contract has none)
SCORE_FLOPS = 27                  # 9 + 3 multiplications, 9 + 2 additions, 3 subtractions, 1 compare


def best(fn, repeats):
    ms = []
    for _ in range(1 + repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[0], min(ms[1:])


def xyz(cloud):
    p = cloud.download().points
    return np.stack([p["x"], p["y"], p["z"]], axis=1).astype(np.float32)


def icp_from(ctx, src, tgt, guess, gate):
    icp = api.IterativeClosestPoint(ctx)
    icp.setMaximumIterations(50)
    icp.setMaxCorrespondenceDistance(gate)
    icp.setInputSource(src)
    icp.setInputTarget(tgt)
    icp.align(guess).close()
    return icp.getFinalTransformation()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="0,20")
    ap.add_argument("--leaves", default="0.06,0.03")
    ap.add_argument("--size", default="N300")
    ap.add_argument("--hypotheses", type=int, default=4096)
    ap.add_argument("--count-hypotheses", type=int, default=262144, help="the transforms repeated up to so many for a second count_inliers line")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_time.jsonl"))
    a = ap.parse_args()
    import sac_ref as R   # tests/sac_ref.py: the numpy scoring
    ctx = api.Context(0)
    ks, kt = (int(v) for v in a.frames.split(","))
    truth = synth.ground_truth(ks, kt, "bench")
    frames = synth.render_frame(ks, a.size, preset="bench"), synth.render_frame(kt, a.size, preset="bench")
    lines = []
    for leaf in (float(v) for v in a.leaves.split(",")):
        src, tgt = (api.DeviceCloud(f, ctx=ctx).voxel_grid(leaf) for f in frames)
        fs, ft = (c.fpfh_cloud(c.normals_cloud(10), 10) for c in (src, tgt))
        corr = fs.feature_correspondences(ft, None, True)
        n = len(corr)
        prm = dict(inlier_threshold=a.threshold, max_iterations=a.hypotheses, seed=1)
        out = {}

        def run_sac():
            out["kept"], out["res"] = src.sac_correspondences(tgt, corr, **prm)
        sac_first, sac_repeat = best(run_sac, a.repeats)
        res = out["res"]
        # the same hypotheses, scored alone: their transforms from the reference's generator
        P, Q, finite = R.pair_points(xyz(src), xyz(tgt), corr)
        hyp = R.hypotheses(api, P, Q, finite, 1, a.hypotheses)
        Ts = np.array([np.full((4, 4), np.nan, np.float32) if t is None else t for t, _ in hyp], np.float32)

        def run_count():
            out["counts"] = src.count_inliers(tgt, corr, Ts, a.threshold)
        cnt_first, cnt_repeat = best(run_count, a.repeats)
        t0 = time.perf_counter()
        want = R.count_inliers(Ts, P, Q, finite, a.threshold)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        bound_ms = n * a.hypotheses * SCORE_FLOPS / PEAK_FLOPS * 1e3
        # ... and repeated to a size at which the kernel, not the call around it, is what is timed
        many = np.tile(Ts, (max(1, a.count_hypotheses // len(Ts)), 1, 1))

        def run_many():
            out["many"] = src.count_inliers(tgt, corr, many, a.threshold)
        many_first, many_repeat = best(run_many, a.repeats)
        many_bound_ms = n * len(many) * SCORE_FLOPS / PEAK_FLOPS * 1e3
        gate = 4 * leaf
        t_icp = icp_from(ctx, src, tgt, res.transform, gate) if res.found else None
        t_id = icp_from(ctx, src, tgt, None, gate)

        def err(T):
            return None if T is None else round(float(np.linalg.norm(np.asarray(T, np.float64) - truth)), 6)
        rec = {"frames": [ks, kt], "size": a.size, "leaf": leaf, "ns": len(src), "nt": len(tgt), "correspondences": n, "hypotheses": a.hypotheses,
               "sac_first_ms": round(sac_first, 3), "sac_repeat_ms": round(sac_repeat, 3), "iterations": res.iterations, "found": res.found,
               "n_inliers": res.n_inliers, "best_hypothesis": res.best_hypothesis,
               "count_first_ms": round(cnt_first, 3), "count_repeat_ms": round(cnt_repeat, 3), "issue_bound_ms": round(bound_ms, 5),
               "fraction_of_issue_bound": round(bound_ms / cnt_repeat, 5), "numpy_count_ms": round(numpy_ms, 1),
               "counts_equal_numpy": bool((out["counts"] == want).all()),
               "many_hypotheses": len(many), "many_count_first_ms": round(many_first, 3), "many_count_repeat_ms": round(many_repeat, 3),
               "many_issue_bound_ms": round(many_bound_ms, 4), "many_fraction_of_issue_bound": round(many_bound_ms / many_repeat, 4),
               "many_counts_equal_numpy": bool((out["many"] == np.tile(want, len(many) // len(Ts))).all()),
               "err_ransac": err(res.transform if res.found else None), "err_ransac_icp": err(t_icp), "err_identity_icp": err(t_id),
               "truth_from_identity": err(np.eye(4))}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        for c in (src, tgt, fs, ft):
            c.close()
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
