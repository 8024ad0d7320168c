"""Host wall time of rsreg_cloud_normals (k = 10, 20, 50) on rendered frames of 50 k, 307 k and 1 M records: the first call and
the best of the repeats, on the frame after PassThrough(z, 0.2, 2.5) and on the raw frame with its pile of missing-depth
records at the origin.  In the same run, on the same frame: rsreg_cloud_knn_mean_distance at mean_k = k - 1 (the value-only
form of the same search), and what a user would otherwise run on the CPU -- cKDTree build + query(k, workers = 16) and a
batched numpy.linalg.eigh of the covariances.

    python tools/normals_time.py [--sizes 50k,N300,N1M] [--repeats 3] [--ks 10,20,50] [--forms passthrough,raw]
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


def cpu_normals(xyz, k):
    from scipy.spatial import cKDTree
    t = xyz[np.isfinite(xyz).all(axis=1)].astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(t)
    t1 = time.perf_counter()
    _, idx = tree.query(t, k, workers=16)
    t2 = time.perf_counter()
    for s in range(0, len(t), 1 << 16):
        d = t[idx[s:s + (1 << 16)]] - t[s:s + (1 << 16), None, :]
        m = d.mean(axis=1)
        np.linalg.eigh(np.einsum("nki,nkj->nij", d, d) / k - m[:, :, None] * m[:, None, :])
    t3 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3


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
    ap.add_argument("--ks", default="10,20,50")
    ap.add_argument("--forms", default="passthrough,raw")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    ctx = api.Context(0)
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
            for k in (int(v) for v in a.ks.split(",")):
                out = api.DeviceCloud(ctx=ctx)

                def run():
                    api._l.check(api._l.lib().rsreg_cloud_normals(ctx.h, dc.h, k, None, out.h), ctx.h)
                    ctx.synchronize()
                first, repeat = best(run, a.repeats)
                sor_first, sor_repeat = best(lambda: dc.knn_mean_distance(k - 1), a.repeats)
                line = {"size": size, "form": form, "records": len(dc), "k": k,
                        "gpu_normals_first_ms": round(first, 3), "gpu_normals_repeat_ms": round(repeat, 3),
                        "gpu_knn_mean_distance_first_ms": round(sor_first, 3), "gpu_knn_mean_distance_repeat_ms": round(sor_repeat, 3),
                        "ratio_repeat": round(repeat / sor_repeat, 2)}
                if not a.no_cpu:
                    build, query, eig = cpu_normals(xyz, k)
                    line.update({"cpu_ckdtree_build_ms": round(build, 1), "cpu_ckdtree_query_ms": round(query, 1), "cpu_cov_eigh_ms": round(eig, 1)})
                print(json.dumps(line), flush=True)
                out.close()


if __name__ == "__main__":
    main()
