"""Point-to-plane ICP (estimation = 1) against staged point-to-point ICP on the synthetic "bench" pairs of 50 k, 307 k and 1 M
records, 5 cm gate, from the identity, the target's normals from rsreg_cloud_normals (k = 10) on the device:

  * host wall time per alignment of 10 fixed iterations and per iteration (the first call and the best of the repeats), for
    point-to-plane and for point-to-point with RSREG_PIPELINE_STAGED, in the same run on the same context;
  * the iteration after which |T - synth.ground_truth|_F stops improving, and the error there, for both (step-wise loop);
  * kernel times of k_plane_reduce against k_cov_reduce, from a `rocprofv3 --kernel-trace --stats` run of this file's
    alignments in a process of its own (--no-profile: left out).

    python tools/plane_time.py [--sizes 50k,N300,N1M] [--repeats 3] [--out profiles/plane_icp_time.jsonl]

One JSON line per size, printed and appended to --out.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rsreg_amd  # noqa: E402,F401
from rsreg_amd import api, synth  # noqa: E402

GATE = 0.05
ITERATIONS = 10
MAX_SWEEP = 40


def make(ctx, plane, tgt, src, nrm):
    icp = api.IterativeClosestPointWithNormals(ctx) if plane else api.IterativeClosestPoint(ctx)
    icp.params = api.icp_params(max_iterations=ITERATIONS, criteria_mode=1, pipeline_mode=0, max_correspondence_distance=GATE,
                                estimation=1 if plane else 0)
    icp.setInputSource(src)
    if plane:
        icp.setInputTarget(tgt, nrm)
    else:
        icp.setInputTarget(tgt)
    return icp


def timed_aligns(icp, ctx, repeats):
    ms = []
    for _ in range(1 + repeats):
        t0 = time.perf_counter()
        icp.align()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[0], min(ms[1:])


def error_sweep(icp, plane, truth):
    """|final - truth|_F after every iteration of the step-wise loop (final composed here in float64: for the curve only)."""
    icp.params.max_iterations = MAX_SWEEP
    icp.begin()
    final = np.eye(4)
    errs = []
    for _ in range(MAX_SWEEP):
        icp.search(want_output=False)
        if plane:
            t, done = icp.update_plane(icp.plane_sums())
        else:
            t, done = icp.update(icp.sums())
        final = t.astype(np.float64) @ final
        errs.append(float(np.linalg.norm(final - truth)))
        if done:
            break
    icp.end()
    icp.params.max_iterations = ITERATIONS
    best = int(np.argmin(errs))
    stop = next((i for i in range(len(errs) - 1) if errs[i + 1] >= errs[i]), len(errs) - 1)
    return {"stops_improving_after": stop + 1, "error_there": errs[stop], "best_iteration": best + 1, "best_error": errs[best],
            "error_after_10": errs[min(ITERATIONS, len(errs)) - 1]}


def kernel_times(size):
    """mean ns of k_plane_reduce and k_cov_reduce over the launches of a profiled child that runs both alignments once"""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--child", "--sizes", size], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if r.returncode != 0:
            return {"profile_error": r.stdout[-500:]}
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for name in ("k_plane_reduce", "k_cov_reduce(", "k_final_reduce"):
                    if "rsreg::" + name in row["Name"]:
                        key = name.rstrip("(")
                        out[key + "_calls"] = int(row["Calls"])
                        out[key + "_mean_us"] = round(float(row["AverageNs"]) / 1e3, 3)
                        out[key + "_min_us"] = round(float(row["MinNs"]) / 1e3, 3)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50k,N300,N1M")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_icp_time.jsonl"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help="(internal) one alignment of each kind, for the kernel trace")
    a = ap.parse_args()
    ctx = api.Context(0)
    for size in a.sizes.split(","):
        tgt = api.DeviceCloud(synth.render_frame(0, size, "bench"), ctx=ctx)
        src = api.DeviceCloud(synth.render_frame(1, size, "bench"), ctx=ctx)
        nrm = tgt.normals_cloud(10)
        ctx.synchronize()
        plane, point = make(ctx, True, tgt, src, nrm), make(ctx, False, tgt, src, nrm)
        if a.child:
            plane.align()
            point.align()
            ctx.synchronize()
            continue
        truth = synth.ground_truth(1, 0, "bench")
        line = {"size": size, "records": len(src), "gate": GATE, "iterations": ITERATIONS}
        for name, icp, is_plane in (("plane", plane, True), ("point_staged", point, False)):
            first, repeat = timed_aligns(icp, ctx, a.repeats)
            line[name + "_align_first_ms"] = round(first, 3)
            line[name + "_align_repeat_ms"] = round(repeat, 3)
            line[name + "_per_iteration_ms"] = round(repeat / ITERATIONS, 4)
            line[name + "_pairs_last"] = int(icp.result.n_correspondences)
            line[name + "_error_after_align"] = float(np.linalg.norm(icp.getFinalTransformation().astype(np.float64) - truth))
            for k, v in error_sweep(icp, is_plane, truth).items():
                line[name + "_" + k] = round(v, 6) if isinstance(v, float) else v
        if not a.no_profile:
            line.update(kernel_times(size))
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        for c in (nrm, src, tgt):
            c.close()


if __name__ == "__main__":
    main()
