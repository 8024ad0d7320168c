"""Host wall time of rsreg_cloud_euclidean_clusters (labels, indices and offsets all asked for) on rendered frames of 50 k, 307 k and
1 M records after PassThrough(z, 0.2, 2.5), at tolerances 0.01, 0.02 and 0.05: the first call of the process and the best of the
repeats.  Beside each, in the same process, rsreg_cloud_radius_count on the same cloud and radius -- the same index and the same
walk without the links and without the ranking: the floor the clustering is measured against.  One JSON line per (size, tolerance);
what profiles/cluster_time.jsonl holds.

    python tools/cluster_time.py [--sizes 50k,N300,N1M] [--tolerances 0.01,0.02,0.05] [--repeats 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rsreg_amd  # noqa: E402,F401
from rsreg_amd import api  # noqa: E402
from rsreg_amd import synth  # noqa: E402


def timed(call, repeats):
    ms = []
    for _ in range(1 + repeats):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[0], min(ms[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50k,N300,N1M")
    ap.add_argument("--tolerances", default="0.01,0.02,0.05")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = api._l.lib()
    ctx = api.Context(0)
    out = open(a.out, "w") if a.out else None
    for size in a.sizes.split(","):
        p = api.PassThrough()
        p.setInputCloud(api.DeviceCloud(synth.render_frame(1, size), ctx=ctx))
        p.setFilterFieldName("z")
        p.setFilterLimits(0.2, 2.5)
        dc = p.filter()
        n = len(dc)
        labels, indices, offsets, counts = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n, np.uint32)
        found = C.c_uint32(0)
        for tol in (float(t) for t in a.tolerances.split(",")):
            params = api.cluster_params(tol)

            def clusters():
                api._l.check(L.rsreg_cloud_euclidean_clusters(ctx.h, dc.h, C.byref(params), labels.ctypes.data, indices.ctypes.data, offsets.ctypes.data,
                                                              n, C.byref(found)), ctx.h)

            def count():
                api._l.check(L.rsreg_cloud_radius_count(ctx.h, dc.h, tol, counts.ctypes.data), ctx.h)

            c_first, c_repeat = timed(clusters, a.repeats)
            r_first, r_repeat = timed(count, a.repeats)
            line = json.dumps({"size": size, "records": n, "tolerance": tol, "clusters": found.value, "largest": int(offsets[1]) if found.value else 0,
                               "mean_neighbours": round(float(counts.mean()), 2),
                               "clusters_first_ms": round(c_first, 3), "clusters_repeat_ms": round(c_repeat, 3),
                               "radius_count_first_ms": round(r_first, 3), "radius_count_repeat_ms": round(r_repeat, 3),
                               "ratio_repeat": round(c_repeat / r_repeat, 2)})
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
