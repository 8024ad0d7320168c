"""SampleConsensusPrerejective on the scenario of tools/sac_time.py: two rendered frames a known LARGE motion apart, VoxelGrid ->
NormalEstimation(10) -> FPFHEstimation(10) -> feature_knn(k) -> prerejective (poses from descriptor neighbours, each scored against
the whole target cloud) -> ICP from that pose.  Per leaf one line: host wall time of rsreg_cloud_prerejective, first call / best
repeat, at each iteration count; the valid hypotheses (the ones that were searched); the wall time of rsreg_cloud_score_transforms
over fixed transforms around the truth; and the Frobenius distance of the pose from the ground truth after the call (with
select_by_inliers, and with PCL's own selection rule), after ICP from it, and after ICP from the identity.  Everything is reported,
nothing asserted.

    python tools/prerej_time.py [--frames 0,20] [--leaves 0.06,0.03,0.015] [--size N300] [--k 5] [--iterations 4096,50000]
                                [--transforms 4096] [--repeats 2] [--out profiles/prerej_time.jsonl]
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


def best(fn, repeats):
    ms = []
    for _ in range(1 + repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[0], min(ms[1:])


def icp_from(ctx, src, tgt, guess, gate):
    icp = api.IterativeClosestPoint(ctx)
    icp.setMaximumIterations(50)
    icp.setMaxCorrespondenceDistance(gate)
    icp.setInputSource(src)
    icp.setInputTarget(tgt)
    icp.align(guess).close()
    return icp.getFinalTransformation()


def around(truth, H, seed=0):
    """(H, 4, 4) float32: the truth disturbed by a rotation of 0 .. 0.05 rad and a shift of 0 .. 0.1; every 7th a random rigid motion"""
    import sac_cases as K   # tests/sac_cases.py: rigid()
    rng = np.random.default_rng(seed)
    out = np.empty((H, 4, 4), np.float32)
    for j in range(H):
        if j % 7 == 6:
            out[j] = K.rigid(rng.normal(size=3), rng.uniform(0, np.pi), rng.uniform(-1, 1, 3))
        else:
            out[j] = K.rigid(rng.normal(size=3), rng.uniform(0, 0.05), rng.normal(size=3) * rng.uniform(0, 0.1) / 3 ** 0.5) @ truth
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="0,20")
    ap.add_argument("--leaves", default="0.06,0.03,0.015")
    ap.add_argument("--size", default="N300")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--iterations", default="4096,50000")
    ap.add_argument("--transforms", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--range-leaves", type=float, default=2.5, help="max_correspondence_distance in leaf sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prerej_time.jsonl"))
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
        fs, ft = (c.fpfh_cloud(c.normals_cloud(10), 10) for c in (src, tgt))
        t0 = time.perf_counter()
        nbr, _ = fs.feature_knn(ft, a.k)
        knn_ms = (time.perf_counter() - t0) * 1e3
        rng_m = a.range_leaves * leaf
        rec = {"frames": [ks, kt], "size": a.size, "leaf": leaf, "ns": len(src), "nt": len(tgt), "k": a.k, "eligible": int((nbr[:, 0] >= 0).sum()),
               "max_correspondence_distance": rng_m, "feature_knn_ms": round(knn_ms, 3), "runs": []}
        out = {}
        for its in (int(v) for v in a.iterations.split(",")):
            prm = dict(max_iterations=its, similarity_threshold=0.9, max_correspondence_distance=rng_m, seed=1)

            def run():
                out["inliers"], out["res"] = src.prerejective(tgt, nbr, select_by_inliers=1, **prm)
            first, repeat = best(run, a.repeats)
            res = out["res"]
            _, pcl = src.prerejective(tgt, nbr, select_by_inliers=0, capacity=0, **prm)
            gate = 4 * leaf
            t_icp = icp_from(ctx, src, tgt, res.transform, gate) if res.found else None
            rec["runs"].append({"iterations": its, "first_ms": round(first, 3), "repeat_ms": round(repeat, 3), "n_valid": res.n_valid, "found": res.found,
                                "n_inliers": res.n_inliers, "best_hypothesis": res.best_hypothesis, "fitness": res.fitness,
                                "err_prerejective": err(res.transform if res.found else None), "err_prerejective_icp": err(t_icp),
                                "pcl_rule_n_inliers": pcl.n_inliers, "pcl_rule_best_hypothesis": pcl.best_hypothesis,
                                "err_pcl_rule": err(pcl.transform if pcl.found else None)})
        Ts = around(truth, a.transforms)

        def run_score():
            out["scores"] = src.score_transforms(tgt, Ts, rng_m)
        sc_first, sc_repeat = best(run_score, a.repeats)
        t_id = icp_from(ctx, src, tgt, None, 4 * leaf)
        rec.update({"score_transforms": a.transforms, "score_first_ms": round(sc_first, 3), "score_repeat_ms": round(sc_repeat, 3),
                    "score_max_count": int(out["scores"][0].max()), "err_identity_icp": err(t_id), "truth_from_identity": err(np.eye(4))})
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
