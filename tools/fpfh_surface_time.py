"""Host wall time of the three search-surface calls -- rsreg_cloud_radius_count_surface, rsreg_cloud_normals_radius_surface and
rsreg_cloud_fpfh_radius_surface -- with VoxelGrid output as the queries and the frame it came from as the surface: the first call
and the best of the repeats, at leaves 0.06 / 0.03 / 0.015 and a radius of 2.5 and 5 leaves, on rendered frames of 307 k and 1 M
records after PassThrough(z, 0.2, 2.5).  The surface's normals are rsreg_cloud_normals(k = 10) of the frame.  Beside each, in the
same run on the same frame, the only other route to the same rows: rsreg_cloud_fpfh_radius on the whole frame.  One line per
(frame, leaf, support) with n_spfh / ns, the share of the surface whose SPFH row the call computed, and the ratio of the two repeats;
no ratio is asserted.  The count call does little beside building the index over the surface: its time is what every call pays for
the build.

    python tools/fpfh_surface_time.py [--sizes N300,N1M] [--leaves 0.06,0.03,0.015] [--supports 2.5,5] [--repeats 2] [--shuffle]
                                      [--out profiles/fpfh_surface_time.jsonl]
--shuffle: the queries in a random order, what a caller with keypoints from elsewhere may hand over (the calls order them by
surface cell themselves).
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
from rsreg_amd import api, synth  # noqa: E402


def best(fn, repeats):
    ms = []
    for _ in range(1 + repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(ms[0], 3), round(min(ms[1:]), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="N300,N1M")
    ap.add_argument("--leaves", default="0.06,0.03,0.015")
    ap.add_argument("--supports", default="2.5,5", help="the radius in leaf sizes")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--shuffle", action="store_true", help="the queries in a random order, not in VoxelGrid's leaf order")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_surface_time.jsonl"))
    a = ap.parse_args()
    ctx = api.Context(0)
    L = api._l.lib()
    lines = []
    for size in a.sizes.split(","):
        p = api.PassThrough()
        p.setInputCloud(api.DeviceCloud(synth.render_frame(1, size), ctx=ctx))
        p.setFilterFieldName("z")
        p.setFilterLimits(0.2, 2.5)
        surface = p.filter()
        nd = surface.normals_cloud(10)
        ns = len(surface)
        out = api.DeviceCloud(ctx=ctx)
        for leaf in (float(v) for v in a.leaves.split(",")):
            queries = surface.voxel_grid(leaf)
            if a.shuffle:
                host = queries.download()
                host.points = host.points[np.random.default_rng(0).permutation(len(host.points))]
                queries.close()
                queries = api.DeviceCloud(host, ctx=ctx)
            nq = len(queries)
            counts = np.zeros(nq, np.uint32)
            for support in (float(v) for v in a.supports.split(",")):
                radius = support * leaf
                n_spfh = C.c_uint64(0)

                def run_count():
                    api._l.check(L.rsreg_cloud_radius_count_surface(ctx.h, queries.h, surface.h, radius, counts.ctypes.data), ctx.h)

                def run_normals():
                    api._l.check(L.rsreg_cloud_normals_radius_surface(ctx.h, queries.h, surface.h, radius, None, out.h), ctx.h)
                    ctx.synchronize()

                def run_fpfh():
                    api._l.check(L.rsreg_cloud_fpfh_radius_surface(ctx.h, queries.h, surface.h, nd.h, radius, out.h, C.byref(n_spfh)), ctx.h)
                    ctx.synchronize()

                def run_whole_frame():
                    api._l.check(L.rsreg_cloud_fpfh_radius(ctx.h, surface.h, nd.h, radius, out.h), ctx.h)
                    ctx.synchronize()

                c_first, c_repeat = best(run_count, a.repeats)
                n_first, n_repeat = best(run_normals, a.repeats)
                f_first, f_repeat = best(run_fpfh, a.repeats)
                nan_rows = int(np.isnan(out.download_fpfh().points["histogram"]).any(axis=1).sum())
                w_first, w_repeat = best(run_whole_frame, a.repeats)
                line = {"size": size, "ns": ns, "leaf": leaf, "nq": nq, "queries_shuffled": bool(a.shuffle), "support_leaves": support, "radius": radius,
                        "neighbours_max": int(counts.max()), "neighbours_mean": round(float(counts.mean()), 1), "nan_rows": nan_rows,
                        "n_spfh": int(n_spfh.value), "n_spfh_share": round(n_spfh.value / ns, 4),
                        "count_surface_first_ms": c_first, "count_surface_repeat_ms": c_repeat,
                        "normals_surface_first_ms": n_first, "normals_surface_repeat_ms": n_repeat,
                        "fpfh_surface_first_ms": f_first, "fpfh_surface_repeat_ms": f_repeat,
                        "fpfh_whole_frame_first_ms": w_first, "fpfh_whole_frame_repeat_ms": w_repeat,
                        "whole_frame_over_surface": round(w_repeat / f_repeat, 2)}
                print(json.dumps(line), flush=True)
                lines.append(line)
            queries.close()
        for c in (out, nd, surface):
            c.close()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
