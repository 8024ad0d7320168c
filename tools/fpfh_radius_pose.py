"""What the radius descriptor is worth to the pose: the pipeline of tools/sac_time.py and tools/prerej_time.py -- the same two rendered
frames a known LARGE motion apart, the same leaves, seeds and thresholds -- once with FPFHEstimation(k = 10) over normals at k = 10,
as those tools run it, and once per support with FPFHEstimationOMP::setRadiusSearch(s leaves) over normals by radius (2 leaves).
Per leaf and descriptor one line: the reciprocal correspondences and how many of them are TRUE (the matched target point lies within
--true-leaves leaves of the source point moved by the ground truth); the Frobenius distance of the pose from the ground truth after
RANSAC over the correspondences, after SampleConsensusPrerejective at each iteration count, and after ICP from each; ICP from the
identity beside them; and the host wall time of the descriptor call.  Everything is reported, nothing asserted.

    python tools/fpfh_radius_pose.py [--frames 0,20] [--leaves 0.06,0.03,0.015] [--size N300] [--supports 2.5,5] [--normals-leaves 2]
                                     [--iterations 4096,50000] [--out profiles/fpfh_radius_pose.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rsreg_amd  # noqa: E402,F401
from rsreg_amd import api  # noqa: E402
from rsreg_amd import synth  # noqa: E402


def xyz(cloud):
    p = cloud.download().points
    return np.stack([p["x"], p["y"], p["z"]], axis=1).astype(np.float64)


def icp_from(ctx, src, tgt, guess, gate):
    icp = api.IterativeClosestPoint(ctx)
    icp.setMaximumIterations(50)
    icp.setMaxCorrespondenceDistance(gate)
    icp.setInputSource(src)
    icp.setInputTarget(tgt)
    icp.align(guess).close()
    return icp.getFinalTransformation()


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="0,20")
    ap.add_argument("--leaves", default="0.06,0.03,0.015")
    ap.add_argument("--size", default="N300")
    ap.add_argument("--supports", default="2.5,5", help="the descriptor's radius in leaf sizes")
    ap.add_argument("--normals-leaves", type=float, default=2.0, help="the radius of the normals under the radius descriptor, in leaf sizes")
    ap.add_argument("--k", type=int, default=5, help="descriptor neighbours a prerejective sample draws from (tools/prerej_time.py)")
    ap.add_argument("--iterations", default="4096,50000")
    ap.add_argument("--hypotheses", type=int, default=4096, help="RANSAC over the correspondences (tools/sac_time.py)")
    ap.add_argument("--threshold", type=float, default=0.05, help="its inlier threshold")
    ap.add_argument("--range-leaves", type=float, default=2.5, help="prerejective's max_correspondence_distance in leaf sizes")
    ap.add_argument("--true-leaves", type=float, default=2.0, help="a match is true within so many leaf sizes of the ground truth")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_radius_pose.jsonl"))
    a = ap.parse_args()
    ctx = api.Context(0)
    ks, kt = (int(v) for v in a.frames.split(","))
    truth = synth.ground_truth(ks, kt, "bench")
    frames = synth.render_frame(ks, a.size, preset="bench"), synth.render_frame(kt, a.size, preset="bench")

    def err(T):
        return None if T is None else round(float(np.linalg.norm(np.asarray(T, np.float64) - truth)), 6)

    lines = []
    for leaf in (float(v) for v in a.leaves.split(",")):
        src, tgt = (api.DeviceCloud(f, ctx=ctx).voxel_grid(leaf) for f in frames)
        ps, pt = xyz(src), xyz(tgt)
        moved = ps @ truth[:3, :3].T + truth[:3, 3]
        gate = 4 * leaf
        id_icp = err(icp_from(ctx, src, tgt, None, gate))
        descriptors = [("k10", None)] + [("radius", float(s)) for s in a.supports.split(",")]
        for kind, support in descriptors:
            def describe(c):
                if kind == "k10":
                    return c.fpfh_cloud(c.normals_cloud(10), 10)
                return c.fpfh_radius_cloud(c.normals_radius_cloud(a.normals_leaves * leaf), support * leaf)
            (fs, ft), first_ms = timed(lambda: (describe(src), describe(tgt)))
            (fs2, ft2), repeat_ms = timed(lambda: (describe(src), describe(tgt)))
            for c in (fs2, ft2):
                c.close()
            valid = [int(np.isfinite(f.download_fpfh().points["histogram"]).all(axis=1).sum()) for f in (fs, ft)]
            corr = fs.feature_correspondences(ft, None, True)
            d = np.linalg.norm(moved[corr["index_query"]] - pt[corr["index_match"]], axis=1)
            rec = {"frames": [ks, kt], "size": a.size, "leaf": leaf, "ns": len(src), "nt": len(tgt), "descriptor": kind,
                   "support_leaves": support, "radius": None if support is None else support * leaf,
                   "normals": "k = 10" if kind == "k10" else "radius %g" % (a.normals_leaves * leaf), "valid_rows": valid,
                   "normals_and_descriptor_both_clouds_first_ms": round(first_ms, 3), "normals_and_descriptor_both_clouds_repeat_ms": round(repeat_ms, 3),
                   "reciprocal_matches": len(corr), "true_matches": int((d <= a.true_leaves * leaf).sum()), "true_within_leaves": a.true_leaves}
            _, res = src.sac_correspondences(tgt, corr, inlier_threshold=a.threshold, max_iterations=a.hypotheses, seed=1)
            t_icp = icp_from(ctx, src, tgt, res.transform, gate) if res.found else None
            rec.update({"ransac_hypotheses": a.hypotheses, "ransac_n_inliers": res.n_inliers, "err_ransac": err(res.transform if res.found else None),
                        "err_ransac_icp": err(t_icp)})
            nbr, _ = fs.feature_knn(ft, a.k)
            rec["prerejective"] = []
            for its in (int(v) for v in a.iterations.split(",")):
                _, pr = src.prerejective(tgt, nbr, select_by_inliers=1, max_iterations=its, similarity_threshold=0.9,
                                         max_correspondence_distance=a.range_leaves * leaf, seed=1)
                t_icp = icp_from(ctx, src, tgt, pr.transform, gate) if pr.found else None
                rec["prerejective"].append({"iterations": its, "n_valid": pr.n_valid, "n_inliers": pr.n_inliers,
                                            "err_prerejective": err(pr.transform if pr.found else None), "err_prerejective_icp": err(t_icp)})
            rec.update({"err_identity_icp": id_icp, "truth_from_identity": err(np.eye(4))})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            for c in (fs, ft):
                c.close()
        for c in (src, tgt):
            c.close()
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
