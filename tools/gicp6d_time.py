"""GICP6D (rsreg_gicp6d_align) beside GICP (rsreg_gicp_align) on the synthetic 307 k "bench" frame pair, 5 cm gate, from the
identity, device clouds, PCL's epsilons and iteration limits, the covariances (k = 20, epsilon = 1e-3) and colours already set:

  * on a profiling context: the device time of one search launch of each alignment -- the 6-D search (k_nn_search6) and the staged
    3-D search of the same pair in the same process -- as ms_nn / n_nn_launches of the alignment's result, and their ratio;
  * on a plain context: host wall time of the whole alignment for both classes (the first call, which builds the 6-D index, and
    the best of the repeats), outer iterations, inner evaluations, pairs and |T - synth.ground_truth|_F;
  * host wall time of rsreg_cloud_lab of one frame.

    python tools/gicp6d_time.py [--size N300] [--repeats 3] [--weight 0.032] [--out profiles/gicp6d_time.jsonl]

One JSON line, printed and appended to --out.  Everything is reported, nothing asserted.
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
K, EPSILON = 20, 1e-3


def make(ctx, cls, src, tgt, cov_s, cov_t, **kw):
    g = cls(ctx, **kw)
    g.setMaxCorrespondenceDistance(GATE)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    g.setSourceCovariances(cov_s)
    g.setTargetCovariances(cov_t)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="N300")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--weight", type=float, default=0.032)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp6d_time.jsonl"))
    a = ap.parse_args()
    f_tgt, f_src = synth.render_frame(0, a.size, "bench"), synth.render_frame(1, a.size, "bench")
    truth = synth.ground_truth(1, 0, "bench")
    line = {"size": a.size, "records": len(f_src.points), "gate": GATE, "lab_weight": a.weight}
    for profiling in (True, False):
        ctx = api.Context(0, profiling=profiling)
        tgt, src = api.DeviceCloud(f_tgt, ctx=ctx), api.DeviceCloud(f_src, ctx=ctx)
        cov_s, cov_t = src.gicp_covariances_cloud(K, EPSILON), tgt.gicp_covariances_cloud(K, EPSILON)
        if not profiling:
            ms = []
            for _ in range(1 + a.repeats):
                t0 = time.perf_counter()
                out = src.lab_cloud()
                ctx.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
                out.close()
            line["cloud_lab_first_ms"], line["cloud_lab_repeat_ms"] = round(ms[0], 3), round(min(ms[1:]), 3)
        regs = (("gicp", make(ctx, api.GeneralizedIterativeClosestPoint, src, tgt, cov_s, cov_t)),
                ("gicp6d", make(ctx, api.GeneralizedIterativeClosestPoint6D, src, tgt, cov_s, cov_t, lab_weight=a.weight)))
        for name, reg in regs:
            ms = []
            for _ in range(1 + a.repeats):
                t0 = time.perf_counter()
                out = reg.align()
                ctx.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
                out.close()
            r = reg.result
            if profiling:
                line[name + "_search_launch_ms"] = round(r.ms_nn / max(1, r.n_nn_launches), 4)
                line[name + "_search_launches"] = int(r.n_nn_launches)
            else:
                T = reg.getFinalTransformation().astype(np.float64)
                line[name + "_align_first_ms"], line[name + "_align_repeat_ms"] = round(ms[0], 3), round(min(ms[1:]), 3)
                line[name + "_iterations"], line[name + "_inner_evaluations"] = int(r.iterations), int(r.inner_evaluations)
                line[name + "_pairs_last"] = int(r.n_correspondences)
                line[name + "_error"] = float(np.linalg.norm(T - truth))
        for c in (cov_s, cov_t, src, tgt):
            c.close()
    line["search_launch_ratio_6d_over_3d"] = round(line["gicp6d_search_launch_ms"] / max(line["gicp_search_launch_ms"], 1e-9), 3)
    line["error_at_identity"] = float(np.linalg.norm(np.eye(4) - truth))
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
