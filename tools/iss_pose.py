"""What a keypoint detector in front of the descriptors is worth to the pose: the rows of tools/fpfh_surface_pose.py (`surface`: FPFH
AT query points OVER the dense frame after PassThrough(z, 0.2, 2.5), the frame's normals by radius) once with the VoxelGrid leaf
centroids as the queries, as that tool runs them (recomputed here), and once with the ISS keypoints of the dense frame
(rsreg_cloud_iss_keypoints, salient / non-max radius = --salient-leaves / --non-max-leaves leaf sizes, PCL's thresholds) in their place.
Per leaf, support and kind of query one line: the number of queries, n_spfh / ns (the share of the frame's records whose SPFH row
the call needed), the reciprocal correspondences and how many of them are TRUE (the matched target point lies within --true-leaves
leaves of the source point moved by the ground truth), and the Frobenius distance of the pose from the ground truth after RANSAC
over the correspondences, after SampleConsensusPrerejective at each iteration count, and after ICP from each -- ICP always between
the two leaf-centroid clouds, so the last column compares starts, not clouds.  Everything is reported, nothing asserted.

    python tools/iss_pose.py [--frames 0,20] [--leaves 0.06,0.03,0.015] [--size N300] [--supports 2.5,5] [--normals-leaves 2]
                             [--salient-leaves 6] [--non-max-leaves 4] [--iterations 4096,50000] [--out profiles/iss_pose.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rsreg_amd  # noqa: E402,F401
from rsreg_amd import api  # noqa: E402
from rsreg_amd import synth  # noqa: E402

from fpfh_surface_pose import icp_from, passthrough, timed, xyz  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="0,20")
    ap.add_argument("--leaves", default="0.06,0.03,0.015")
    ap.add_argument("--size", default="N300")
    ap.add_argument("--supports", default="2.5,5", help="the descriptor's radius in leaf sizes")
    ap.add_argument("--normals-leaves", type=float, default=2.0, help="the radius of the normals, in leaf sizes")
    ap.add_argument("--salient-leaves", type=float, default=6.0)
    ap.add_argument("--non-max-leaves", type=float, default=4.0)
    ap.add_argument("--k", type=int, default=5, help="descriptor neighbours a prerejective sample draws from")
    ap.add_argument("--iterations", default="4096,50000")
    ap.add_argument("--hypotheses", type=int, default=4096, help="RANSAC over the correspondences")
    ap.add_argument("--threshold", type=float, default=0.05, help="its inlier threshold")
    ap.add_argument("--range-leaves", type=float, default=2.5, help="prerejective's max_correspondence_distance in leaf sizes")
    ap.add_argument("--true-leaves", type=float, default=2.0, help="a match is true within so many leaf sizes of the ground truth")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iss_pose.jsonl"))
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
        leaf_src, leaf_tgt = (c.voxel_grid(leaf) for c in raw)
        gate = 4 * leaf
        id_icp = err(icp_from(ctx, leaf_src, leaf_tgt, None, gate))
        dense_normals = [c.normals_radius_cloud(a.normals_leaves * leaf) for c in dense]
        iss, iss_ms = timed(lambda: [c.iss_keypoints(salient_radius=a.salient_leaves * leaf, non_max_radius=a.non_max_leaves * leaf)[0] for c in dense])
        for support in (float(s) for s in a.supports.split(",")):
            for queries, (src, tgt) in (("leaf_centroids", (leaf_src, leaf_tgt)), ("iss_keypoints", iss)):
                rec = {"frames": [ks, kt], "size": a.size, "leaf": leaf, "queries": queries, "ns": len(src), "nt": len(tgt),
                       "support_leaves": support, "radius": support * leaf, "normals_radius": a.normals_leaves * leaf,
                       "dense_records": [len(c) for c in dense], "err_identity_icp": id_icp, "truth_from_identity": err(np.eye(4))}
                if queries == "iss_keypoints":
                    rec.update({"salient_radius": a.salient_leaves * leaf, "non_max_radius": a.non_max_leaves * leaf, "iss_both_frames_ms": round(iss_ms, 3)})
                if min(len(src), len(tgt)) < max(3, a.k):
                    rec["skipped"] = "fewer queries than a sample needs"
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
                    continue
                fs = ft = None
                try:
                    ps, pt = xyz(src), xyz(tgt)
                    moved = ps @ truth[:3, :3].T + truth[:3, 3]
                    n_spfh = []

                    def describe(c, which):
                        out, n = c.fpfh_radius_surface_cloud(dense[which], dense_normals[which], support * leaf, n_spfh=True)
                        n_spfh.append(n)
                        return out
                    (fs, ft), first_ms = timed(lambda: (describe(src, 0), describe(tgt, 1)))
                    valid = [int(np.isfinite(f.download_fpfh().points["histogram"]).all(axis=1).sum()) for f in (fs, ft)]
                    corr = fs.feature_correspondences(ft, None, True)
                    d = np.linalg.norm(moved[corr["index_query"]] - pt[corr["index_match"]], axis=1)
                    rec.update({"valid_rows": valid, "n_spfh": n_spfh[:2], "n_spfh_share": [round(n_spfh[i] / max(len(dense[i]), 1), 4) for i in (0, 1)],
                                "descriptor_both_clouds_first_ms": round(first_ms, 3), "reciprocal_matches": len(corr),
                                "true_matches": int((d <= a.true_leaves * leaf).sum()), "true_within_leaves": a.true_leaves})
                    res = None
                    if len(corr) >= 3:
                        _, res = src.sac_correspondences(tgt, corr, inlier_threshold=a.threshold, max_iterations=a.hypotheses, seed=1)
                    found = res is not None and res.found
                    t_icp = icp_from(ctx, leaf_src, leaf_tgt, res.transform, gate) if found else None
                    rec.update({"ransac_hypotheses": a.hypotheses, "ransac_n_inliers": res.n_inliers if res is not None else None,
                                "err_ransac": err(res.transform if found else None), "err_ransac_icp": err(t_icp)})
                    nbr, _ = fs.feature_knn(ft, a.k)
                    rec["prerejective"] = []
                    for its in (int(v) for v in a.iterations.split(",")):
                        _, pr = src.prerejective(tgt, nbr, select_by_inliers=1, max_iterations=its, similarity_threshold=0.9,
                                                 max_correspondence_distance=a.range_leaves * leaf, seed=1)
                        t_icp = icp_from(ctx, leaf_src, leaf_tgt, pr.transform, gate) if pr.found else None
                        rec["prerejective"].append({"iterations": its, "n_valid": pr.n_valid, "n_inliers": pr.n_inliers,
                                                    "err_prerejective": err(pr.transform if pr.found else None), "err_prerejective_icp": err(t_icp)})
                except api._l.RsregError as e:      # (a stage that refuses so few queries: reported, the line is kept)
                    rec["refused"] = str(e)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                for c in (fs, ft):
                    if c is not None:
                        c.close()
        for c in [leaf_src, leaf_tgt] + dense_normals + list(iss):
            c.close()
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
