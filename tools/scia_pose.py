"""What SampleConsensusInitialAlignment makes of the descriptors: the rows of tools/fpfh_surface_pose.py (frames, leaves, supports,
seeds and thresholds; descriptors over the downsampled cloud alone and AT the leaf centroids OVER the dense frame), with RANSAC over
the reciprocal correspondences and SampleConsensusPrerejective recomputed in the same run and, beside them, SAC-IA at each iteration
count: truncated error, thr = (--range-leaves leaves)^2, min_sample_distance --sample-leaves leaves, over the same table of k
descriptor neighbours prerejective draws from.  Per row the Frobenius distance of the pose from the ground truth after each
estimator and after ICP from it; ICP from the identity beside them.  Everything is reported, nothing asserted.

    python tools/scia_pose.py [--frames 0,20] [--leaves 0.06,0.03,0.015] [--size N300] [--supports 2.5,5] [--normals-leaves 2]
                              [--iterations 4096,50000] [--scia-iterations 1000,4096] [--out profiles/scia_pose.jsonl]
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
from fpfh_surface_pose import icp_from, passthrough, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="0,20")
    ap.add_argument("--leaves", default="0.06,0.03,0.015")
    ap.add_argument("--size", default="N300")
    ap.add_argument("--supports", default="2.5,5", help="the descriptor's radius in leaf sizes")
    ap.add_argument("--normals-leaves", type=float, default=2.0, help="the radius of the normals, in leaf sizes")
    ap.add_argument("--k", type=int, default=5, help="descriptor neighbours a sample draws from")
    ap.add_argument("--iterations", default="4096,50000", help="prerejective's")
    ap.add_argument("--scia-iterations", default="1000,4096")
    ap.add_argument("--hypotheses", type=int, default=4096, help="RANSAC over the correspondences (tools/sac_time.py)")
    ap.add_argument("--threshold", type=float, default=0.05, help="its inlier threshold")
    ap.add_argument("--range-leaves", type=float, default=2.5, help="prerejective's max_correspondence_distance in leaf sizes; SAC-IA's thr is its square")
    ap.add_argument("--sample-leaves", type=float, default=10.0, help="SAC-IA's min_sample_distance in leaf sizes")
    ap.add_argument("--basin", type=float, default=0.15, help="a pose counts as inside ICP's basin when ICP from it ends within this of the truth")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scia_pose.jsonl"))
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
        gate = 4 * leaf
        id_icp = err(icp_from(ctx, src, tgt, None, gate))
        dense_normals = [c.normals_radius_cloud(a.normals_leaves * leaf) for c in dense]
        for support in (float(s) for s in a.supports.split(",")):
            for over in ("downsampled", "surface"):
                def describe(c, which):
                    if over == "downsampled":
                        return c.fpfh_radius_cloud(c.normals_radius_cloud(a.normals_leaves * leaf), support * leaf)
                    return c.fpfh_radius_surface_cloud(dense[which], dense_normals[which], support * leaf)
                fs, ft = describe(src, 0), describe(tgt, 1)
                corr = fs.feature_correspondences(ft, None, True)
                rec = {"frames": [ks, kt], "size": a.size, "leaf": leaf, "ns": len(src), "nt": len(tgt), "descriptor_over": over, "support_leaves": support,
                       "k": a.k, "reciprocal_matches": len(corr)}
                _, res = src.sac_correspondences(tgt, corr, inlier_threshold=a.threshold, max_iterations=a.hypotheses, seed=1)
                t_icp = icp_from(ctx, src, tgt, res.transform, gate) if res.found else None
                rec.update({"ransac_hypotheses": a.hypotheses, "err_ransac": err(res.transform if res.found else None), "err_ransac_icp": err(t_icp)})
                nbr, _ = fs.feature_knn(ft, a.k)
                rec["eligible"] = int((nbr[:, 0] >= 0).sum())
                rec["prerejective"] = []
                for its in (int(v) for v in a.iterations.split(",")):
                    _, pr = src.prerejective(tgt, nbr, select_by_inliers=1, max_iterations=its, similarity_threshold=0.9,
                                             max_correspondence_distance=a.range_leaves * leaf, seed=1)
                    t_icp = icp_from(ctx, src, tgt, pr.transform, gate) if pr.found else None
                    rec["prerejective"].append({"iterations": its, "n_valid": pr.n_valid, "err_prerejective": err(pr.transform if pr.found else None),
                                                "err_prerejective_icp": err(t_icp)})
                rec["initial_alignment"] = []
                for its in (int(v) for v in a.scia_iterations.split(",")):
                    ia, ms = timed(lambda: src.initial_alignment(tgt, nbr, max_iterations=its, max_correspondence_distance=(a.range_leaves * leaf) ** 2,
                                                                 min_sample_distance=a.sample_leaves * leaf, seed=1))
                    t_icp = icp_from(ctx, src, tgt, ia.transform, gate) if ia.found else None
                    rec["initial_alignment"].append({"iterations": its, "n_valid": ia.n_valid, "error": ia.error, "ms": round(ms, 3),
                                                     "err_initial_alignment": err(ia.transform if ia.found else None), "err_initial_alignment_icp": err(t_icp)})
                rec.update({"err_identity_icp": id_icp, "truth_from_identity": err(np.eye(4))})
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                for c in (fs, ft):
                    c.close()
        for c in [src, tgt] + dense_normals:
            c.close()

    def inside(v):
        return v is not None and v <= a.basin

    summary = {"rows": len(lines), "basin": a.basin, "ransac_inside": sum(inside(r["err_ransac_icp"]) for r in lines)}
    for j, its in enumerate(a.iterations.split(",")):
        summary["prerejective_%s_inside" % its] = sum(inside(r["prerejective"][j]["err_prerejective_icp"]) for r in lines)
    for j, its in enumerate(a.scia_iterations.split(",")):
        summary["initial_alignment_%s_inside" % its] = sum(inside(r["initial_alignment"][j]["err_initial_alignment_icp"]) for r in lines)
    print(json.dumps({"summary": summary}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
            f.write(json.dumps({"summary": summary}) + "\n")


if __name__ == "__main__":
    main()
