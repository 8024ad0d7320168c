"""GICP (rsreg_gicp_align) beside point-to-point and point-to-plane ICP on the synthetic "bench" pairs of 50 k, 307 k and 1 M
records, 5 cm gate, from the identity, everything on device clouds of one context:

  * host wall time of rsreg_cloud_gicp_covariances (k = 20, epsilon = 1e-3) of the source and of the target (the first call and
    the best of the repeats);
  * host wall time of a GICP alignment with PCL's epsilons and iteration limits (the covariances already set), its outer
    iterations, inner evaluations and |T - synth.ground_truth|_F;
  * in the same run, from the same guess: the point-to-point (RSREG_PIPELINE_STAGED) and the point-to-plane alignment of the same
    pair, 10 fixed iterations each, the target's normals from rsreg_cloud_normals (k = 10), with their wall time and error.

    python tools/gicp_time.py [--sizes 50k,N300,N1M] [--repeats 3] [--out profiles/gicp_time.jsonl]

One JSON line per size, printed and appended to --out.  Everything is reported, nothing asserted.
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
from rsreg_amd import api, synth  # noqa: E402

GATE = 0.05
ITERATIONS = 10
K, EPSILON = 20, 1e-3


def timed(ctx, repeats, call):
    ms = []
    for _ in range(1 + repeats):
        t0 = time.perf_counter()
        out = call()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        if isinstance(out, api.DeviceCloud):
            out.close()
    return round(ms[0], 3), round(min(ms[1:]), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50k,N300,N1M")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp_time.jsonl"))
    a = ap.parse_args()
    ctx = api.Context(0)
    for size in a.sizes.split(","):
        tgt = api.DeviceCloud(synth.render_frame(0, size, "bench"), ctx=ctx)
        src = api.DeviceCloud(synth.render_frame(1, size, "bench"), ctx=ctx)
        truth = synth.ground_truth(1, 0, "bench")
        ctx.synchronize()
        line = {"size": size, "records": len(src), "gate": GATE, "k": K, "epsilon": EPSILON}
        for name, cloud in (("source", src), ("target", tgt)):
            first, best = timed(ctx, a.repeats, lambda cloud=cloud: cloud.gicp_covariances_cloud(K, EPSILON))
            line["covariances_%s_first_ms" % name], line["covariances_%s_repeat_ms" % name] = first, best
        cov_s, cov_t = src.gicp_covariances_cloud(K, EPSILON), tgt.gicp_covariances_cloud(K, EPSILON)
        nrm = tgt.normals_cloud(10)
        gicp = api.GeneralizedIterativeClosestPoint(ctx)
        gicp.setMaxCorrespondenceDistance(GATE)
        gicp.setInputSource(src)
        gicp.setInputTarget(tgt)
        gicp.setSourceCovariances(cov_s)
        gicp.setTargetCovariances(cov_t)
        point = api.IterativeClosestPoint(ctx)
        plane = api.IterativeClosestPointWithNormals(ctx)
        for icp, est in ((point, 0), (plane, 1)):
            icp.params = api.icp_params(max_iterations=ITERATIONS, criteria_mode=1, pipeline_mode=0, max_correspondence_distance=GATE, estimation=est)
            icp.setInputSource(src)
        point.setInputTarget(tgt)
        plane.setInputTarget(tgt, nrm)
        for name, reg in (("gicp", gicp), ("point_staged", point), ("plane", plane)):
            first, best = timed(ctx, a.repeats, reg.align)
            T = reg.getFinalTransformation().astype(np.float64)
            line[name + "_align_first_ms"], line[name + "_align_repeat_ms"] = first, best
            line[name + "_iterations"] = int(reg.result.iterations)
            line[name + "_pairs_last"] = int(reg.result.n_correspondences)
            line[name + "_error"] = float(np.linalg.norm(T - truth))
        line["gicp_inner_evaluations"] = int(gicp.result.inner_evaluations)
        line["gicp_ms_per_evaluation"] = round(line["gicp_align_repeat_ms"] / max(1, gicp.result.inner_evaluations + gicp.result.iterations), 4)
        line["error_at_identity"] = float(np.linalg.norm(np.eye(4) - truth))
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        for c in (nrm, cov_s, cov_t, src, tgt):
            c.close()


if __name__ == "__main__":
    main()
