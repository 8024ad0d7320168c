"""Host wall time of the three radius calls -- rsreg_cloud_radius_count, rsreg_cloud_radius_outlier_removal (min_neighbors 10) and
rsreg_cloud_normals_radius -- at r = 0.01, 0.03 and 0.1 on rendered frames of 50 k, 307 k and 1 M records: the first call and the
best of the repeats, on the frame after PassThrough(z, 0.2, 2.5) and on the raw frame, whose pile of missing-depth records at the
origin is the expensive case (every record of the pile reads the whole pile; nothing is approximated).  In the same run, on the
same frame: the repeat of rsreg_cloud_normals(k = 10) and of rsreg_cloud_knn_mean_distance(50), the k-NN calls they stand beside,
and what a user would otherwise run on the CPU -- cKDTree build + query_ball_point(r, return_length, workers = 16).

    python tools/radius_time.py [--sizes 50k,N300,N1M] [--repeats 3] [--radii 0.01,0.03,0.1] [--forms passthrough,raw] [--out profiles/radius_time.jsonl]
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


def cpu_counts(xyz, radius):
    from scipy.spatial import cKDTree
    t = xyz[np.isfinite(xyz).all(axis=1)].astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(t)
    t1 = time.perf_counter()
    n = tree.query_ball_point(t, radius, return_length=True, workers=16)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, int(n.max()), float(n.mean())


def best(fn, repeats):
    ms = []
    for _ in range(1 + repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[0], min(ms[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50k,N300,N1M")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--radii", default="0.01,0.03,0.1")
    ap.add_argument("--forms", default="passthrough,raw")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_time.jsonl"))
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    ctx = api.Context(0)
    L = api._l.lib()
    lines = []
    for size in a.sizes.split(","):
        raw = synth.render_frame(1, size)
        d_raw = api.DeviceCloud(raw, ctx=ctx)
        p = api.PassThrough()
        p.setInputCloud(d_raw)
        p.setFilterFieldName("z")
        p.setFilterLimits(0.2, 2.5)
        d_pass = p.filter()
        for form, dc in (("passthrough", d_pass), ("raw", d_raw)):
            if form not in a.forms.split(","):
                continue
            xyz = dc.download().xyz
            knn_out = api.DeviceCloud(ctx=ctx)

            def run_knn_normals():
                api._l.check(L.rsreg_cloud_normals(ctx.h, dc.h, 10, None, knn_out.h), ctx.h)
                ctx.synchronize()
            _, knn_normals = best(run_knn_normals, a.repeats)
            _, knn_mean = best(lambda: dc.knn_mean_distance(50), a.repeats)
            knn_out.close()
            for radius in (float(v) for v in a.radii.split(",")):
                out, kept = api.DeviceCloud(ctx=ctx), api.DeviceCloud(ctx=ctx)
                counts = np.zeros(len(dc), np.uint32)

                def run_count():
                    api._l.check(L.rsreg_cloud_radius_count(ctx.h, dc.h, radius, counts.ctypes.data), ctx.h)

                def run_ror():
                    api._l.check(L.rsreg_cloud_radius_outlier_removal(ctx.h, dc.h, radius, 10, 0, 0, kept.h, None), ctx.h)
                    ctx.synchronize()

                def run_normals():
                    api._l.check(L.rsreg_cloud_normals_radius(ctx.h, dc.h, radius, None, out.h), ctx.h)
                    ctx.synchronize()
                c_first, c_repeat = best(run_count, a.repeats)
                r_first, r_repeat = best(run_ror, a.repeats)
                n_first, n_repeat = best(run_normals, a.repeats)
                line = {"size": size, "form": form, "records": len(dc), "radius": radius,
                        "neighbours_max": int(counts.max()), "neighbours_mean": round(float(counts[counts > 0].mean()), 2), "ror_kept": len(kept),
                        "gpu_radius_count_first_ms": round(c_first, 3), "gpu_radius_count_repeat_ms": round(c_repeat, 3),
                        "gpu_ror_first_ms": round(r_first, 3), "gpu_ror_repeat_ms": round(r_repeat, 3),
                        "gpu_normals_radius_first_ms": round(n_first, 3), "gpu_normals_radius_repeat_ms": round(n_repeat, 3),
                        "gpu_normals_k10_repeat_ms": round(knn_normals, 3), "gpu_knn_mean_distance_50_repeat_ms": round(knn_mean, 3)}
                if not a.no_cpu:
                    build, query, cmax, cmean = cpu_counts(xyz, radius)
                    line.update({"cpu_ckdtree_build_ms": round(build, 1), "cpu_query_ball_point_ms": round(query, 1)})
                print(json.dumps(line), flush=True)
                lines.append(line)
                out.close()
                kept.close()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
