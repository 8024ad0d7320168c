"""What descriptors over the dense frame are worth to the pose: the frames, leaves, seeds and thresholds of tools/fpfh_radius_pose.py,
once with normals and FPFH estimated on the downsampled cloud alone (`downsampled`: what that tool runs, recomputed here) and once
AT the leaf centroids OVER the dense frame (`surface`: setSearchSurface): the frame's normals by radius (--normals-leaves leaves) on
the frame after PassThrough(z, 0.2, 2.5), then rsreg_cloud_fpfh_radius_surface with the centroids as the queries.  The centroids
are those of the raw frame, as in that tool; the one at the missing-depth pile has no neighbour in the filtered frame and gets a
NaN row, which matching leaves out.
Per leaf, support and source of the descriptor one line: the reciprocal correspondences and how many of them are TRUE (the matched
target point lies within --true-leaves leaves of the source point moved by the ground truth); the Frobenius distance of the pose from
the ground truth after RANSAC over the correspondences, after SampleConsensusPrerejective at each iteration count, and after ICP from
each; ICP from the identity beside them; and the host wall time of the descriptor calls.  Everything is reported, nothing asserted.

    python tools/fpfh_surface_pose.py [--frames 0,20] [--leaves 0.06,0.03,0.015] [--size N300] [--supports 2.5,5] [--normals-leaves 2]
                                      [--iterations 4096,50000] [--out profiles/fpfh_surface_pose.jsonl]
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


def passthrough(cloud):
    p = api.PassThrough()
    p.setInputCloud(cloud)
    p.setFilterFieldName("z")
    p.setFilterLimits(0.2, 2.5)
    return p.filter()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="0,20")
    ap.add_argument("--leaves", default="0.06,0.03,0.015")
    ap.add_argument("--size", default="N300")
    ap.add_argument("--supports", default="2.5,5", help="the descriptor's radius in leaf sizes")
    ap.add_argument("--normals-leaves", type=float, default=2.0, help="the radius of the normals, in leaf sizes")
    ap.add_argument("--k", type=int, default=5, help="descriptor neighbours a prerejective sample draws from (tools/prerej_time.py)")
    ap.add_argument("--iterations", default="4096,50000")
    ap.add_argument("--hypotheses", type=int, default=4096, help="RANSAC over the correspondences (tools/sac_time.py)")
    ap.add_argument("--threshold", type=float, default=0.05, help="its inlier threshold")
    ap.add_argument("--range-leaves", type=float, default=2.5, help="prerejective's max_correspondence_distance in leaf sizes")
    ap.add_argument("--true-leaves", type=float, default=2.0, help="a match is true within so many leaf sizes of the ground truth")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_surface_pose.jsonl"))
    a = ap.parse_args()
    ctx = api.Context(0)
    ks, kt = (int(v) for v in a.frames.split(","))
    truth = synth.ground_truth(ks, kt, "bench")
    raw = [api.DeviceCloud(synth.render_frame(k, a.size, preset="bench"), ctx=ctx) for k in (ks, kt)]
    dense = [passthrough(c) for c in raw]

    def err(T):
        return None if T is None else round(float(np.linalg.norm(np.asarray(T, np.float64) - truth)), 6)

    lines = []
    for leaf in (float(v) for v in a.leaves.split(",")):
        src, tgt = (c.voxel_grid(leaf) for c in raw)
        ps, pt = xyz(src), xyz(tgt)
        moved = ps @ truth[:3, :3].T + truth[:3, 3]
        gate = 4 * leaf
        id_icp = err(icp_from(ctx, src, tgt, None, gate))
        dense_normals, dense_normals_ms = timed(lambda: [c.normals_radius_cloud(a.normals_leaves * leaf) for c in dense])
        for support in (float(s) for s in a.supports.split(",")):
            for over in ("downsampled", "surface"):
                spfh_rows = []

                def describe(c, which):
                    if over == "downsampled":
                        return c.fpfh_radius_cloud(c.normals_radius_cloud(a.normals_leaves * leaf), support * leaf)
                    out, n_spfh = c.fpfh_radius_surface_cloud(dense[which], dense_normals[which], support * leaf, n_spfh=True)
                    spfh_rows.append(n_spfh)
                    return out
                (fs, ft), first_ms = timed(lambda: (describe(src, 0), describe(tgt, 1)))
                (fs2, ft2), repeat_ms = timed(lambda: (describe(src, 0), describe(tgt, 1)))
                for c in (fs2, ft2):
                    c.close()
                valid = [int(np.isfinite(f.download_fpfh().points["histogram"]).all(axis=1).sum()) for f in (fs, ft)]
                corr = fs.feature_correspondences(ft, None, True)
                d = np.linalg.norm(moved[corr["index_query"]] - pt[corr["index_match"]], axis=1)
                rec = {"frames": [ks, kt], "size": a.size, "leaf": leaf, "ns": len(src), "nt": len(tgt), "descriptor_over": over,
                       "support_leaves": support, "radius": support * leaf, "normals_radius": a.normals_leaves * leaf, "valid_rows": valid,
                       "dense_records": [len(c) for c in dense] if over == "surface" else None,
                       "n_spfh": spfh_rows[:2] if over == "surface" else None,
                       "dense_normals_both_frames_ms": round(dense_normals_ms, 3) if over == "surface" else None,
                       "descriptor_both_clouds_first_ms": round(first_ms, 3), "descriptor_both_clouds_repeat_ms": round(repeat_ms, 3),
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
        for c in [src, tgt] + dense_normals:
            c.close()
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
