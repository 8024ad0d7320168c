"""Host wall time of rsreg_cloud_sor (mean_k = 50, 1.5 sigma) on rendered frames of 50 k, 307 k and 1 M records: the first
call of the process and the best of the repeats, on the frame after PassThrough(z, 0.2, 2.5) and on the raw frame with its
pile of missing-depth records at the origin -- next to the CPU search a user would otherwise run on the same frame in the
same process, cKDTree.query(k = mean_k + 1, workers = 16) (build and query; the distances' sums and the filter not counted).
The GPU call must come in under it.

    python tools/sor_time.py [--sizes 50k,N300,N1M] [--repeats 5] [--mean-k 50]
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


def cpu_search(xyz, k):
    from scipy.spatial import cKDTree
    t = xyz[np.isfinite(xyz).all(axis=1)].astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(t)
    t1 = time.perf_counter()
    tree.query(t, k + 1, workers=16)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50k,N300,N1M")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mean-k", type=int, default=50)
    a = ap.parse_args()
    ctx = api.Context(0)
    for size in a.sizes.split(","):
        raw = synth.render_frame(1, size)
        d_raw = api.DeviceCloud(raw, ctx=ctx)
        p = api.PassThrough()
        p.setInputCloud(d_raw)
        p.setFilterFieldName("z")
        p.setFilterLimits(0.2, 2.5)
        t0 = time.perf_counter()
        d_pass = p.filter()
        ms_pass = (time.perf_counter() - t0) * 1e3
        for form, dc in (("passthrough", d_pass), ("raw", d_raw)):
            sor = api.StatisticalOutlierRemoval()
            sor.setInputCloud(dc)
            sor.setMeanK(a.mean_k)
            sor.setStddevMulThresh(1.5)
            ms = []
            for _ in range(1 + a.repeats):
                t0 = time.perf_counter()
                out = sor.filter()
                ms.append((time.perf_counter() - t0) * 1e3)
            build, query = cpu_search(dc.download().xyz, a.mean_k)
            print(json.dumps({"size": size, "form": form, "records": len(dc), "kept": len(out), "threshold": sor.stats.threshold,
                              "gpu_sor_first_ms": round(ms[0], 3), "gpu_sor_repeat_ms": round(min(ms[1:]), 3),
                              "gpu_passthrough_ms": round(ms_pass, 3), "cpu_ckdtree_build_ms": round(build, 1),
                              "cpu_ckdtree_query_ms": round(query, 1), "mean_k": a.mean_k}), flush=True)


if __name__ == "__main__":
    main()
