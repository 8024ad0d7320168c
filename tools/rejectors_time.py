"""What the ICP rejector chain (include/rsreg.h: rsreg_icp_set_rejectors) costs per staged iteration, on the synthetic "bench"
pairs of 50 k, 307 k and 1 M records, 5 cm gate, from the identity, 10 fixed iterations, clouds and normals resident in HBM:

  * host wall time per alignment (ends in a synchronise) and per iteration for: no chain (staged), the fused pipeline,
    trim_overlap_ratio = 0.8 alone, every rejector kind alone, [ONE_TO_ONE, MEDIAN_DISTANCE] and [SURFACE_NORMAL, ONE_TO_ONE,
    MEDIAN_DISTANCE] -- one ICP object on one context, the configurations taken in turn within every repeat, so that a drift
    of the machine falls on all of them alike; the best and the median of the repeats;
  * kernel times of the chain's kernels (k_rej_*, k_trim_*, the radix sort's passes) from a `rocprofv3 --kernel-trace --stats`
    run of a child process that aligns once with [3, 2, 1] and once with [4] (--no-profile: left out).

The median's radix select is the form the library keeps; a sort-based median would be the kernel sequence of the TRIMMED entry
(keys, the library's 64-bit radix sort, one pass over the order), so "trimmed" here is that form's figure.

    python tools/rejectors_time.py [--sizes 50k,N300,N1M] [--repeats 7] [--out profiles/rejectors_time.jsonl]

One JSON line per size, printed and appended to --out.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rsreg_amd  # noqa: E402,F401
from rsreg_amd import api, synth  # noqa: E402

GATE = 0.05
ITERATIONS = 10
M, O, S, T = (api.CorrespondenceRejectorMedianDistance, api.CorrespondenceRejectorOneToOne, api.CorrespondenceRejectorSurfaceNormal,
              api.CorrespondenceRejectorTrimmed)
# name -> (pipeline_mode, trim_overlap_ratio, chain)
CONFIGS = {
    "staged": (0, 0.0, []),
    "fused": (1, 0.0, []),
    "trim_ratio": (0, 0.8, []),
    "median": (0, 0.0, [lambda: M(1.0)]),
    "one_to_one": (0, 0.0, [O]),
    "normal": (0, 0.0, [lambda: S(0.7)]),
    "trimmed": (0, 0.0, [lambda: T(0.8)]),
    "one_to_one,median": (0, 0.0, [O, lambda: M(1.0)]),
    "normal,one_to_one,median": (0, 0.0, [lambda: S(0.7), O, lambda: M(1.0)]),
}


def configure(icp, name):
    pipeline, ratio, chain = CONFIGS[name]
    icp.params.pipeline_mode = pipeline
    icp.params.trim_overlap_ratio = ratio
    icp.clearCorrespondenceRejectors()
    for make in chain:
        icp.addCorrespondenceRejector(make())


def align_ms(icp, ctx):
    t0 = time.perf_counter()
    out = icp.align()
    ctx.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    out.close()
    return ms


def kernel_times(size):
    """mean us per launch of the chain's kernels, over a profiled child's two alignments"""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--child", "--sizes", size], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if r.returncode != 0:
            return {"profile_error": r.stdout[-500:]}
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row["Name"]
                if not any(k in name for k in ("k_rej_", "k_trim_", "radix32", "k_corr_weights", "k_rotate_normals", "k_restart_normals",
                                               "k_cov_reduce_w", "k_nn_search")):
                    continue
                key = name.split("rsreg::")[-1].split("(")[0]
                out[key] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 3), "min_us": round(float(row["MinNs"]) / 1e3, 3)}
        return {"kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50k,N300,N1M")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rejectors_time.jsonl"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help="(internal) one alignment with [3, 2, 1] and one with [4], for the kernel trace")
    a = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    ctx = api.Context(0)
    for size in a.sizes.split(","):
        tgt = api.DeviceCloud(synth.render_frame(0, size, "bench"), ctx=ctx)
        src = api.DeviceCloud(synth.render_frame(1, size, "bench"), ctx=ctx)
        tgt_n, src_n = tgt.normals_cloud(10), src.normals_cloud(10)
        ctx.synchronize()
        icp = api.IterativeClosestPoint(ctx)
        icp.params = api.icp_params(max_iterations=ITERATIONS, criteria_mode=1, max_correspondence_distance=GATE)
        icp.setInputSource(src)
        icp.setInputTarget(tgt)
        icp.setInputSourceNormals(src_n)
        icp.setInputTargetNormals(tgt_n)
        if a.child:
            for name in ("normal,one_to_one,median", "trimmed"):
                configure(icp, name)
                align_ms(icp, ctx)
            continue
        line = {"size": size, "records": len(src), "gate": GATE, "iterations": ITERATIONS, "repeats": a.repeats}
        ms = {name: [] for name in CONFIGS}
        pairs = {}
        for name in CONFIGS:            # warm-up: every configuration once (code objects, buffers, the normals' way in)
            configure(icp, name)
            align_ms(icp, ctx)
            pairs[name] = int(icp.result.n_correspondences)
        for _ in range(a.repeats):
            for name in CONFIGS:
                configure(icp, name)
                ms[name].append(align_ms(icp, ctx))
        for name in CONFIGS:
            line[name] = {"align_best_ms": round(min(ms[name]), 4), "align_median_ms": round(statistics.median(ms[name]), 4),
                          "per_iteration_best_us": round(min(ms[name]) / ITERATIONS * 1e3, 2),
                          "per_iteration_median_us": round(statistics.median(ms[name]) / ITERATIONS * 1e3, 2), "pairs_last": pairs[name]}
        if not a.no_profile:
            line.update(kernel_times(size))
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        for c in (tgt_n, src_n, src, tgt):
            c.close()


if __name__ == "__main__":
    main()
