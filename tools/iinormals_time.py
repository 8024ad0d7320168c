"""Host wall time of rsreg_cloud_integral_normals (PCL's defaults: AVERAGE_3D_GRADIENT, 0.02, 10) on rendered frames of 50 k,
307 k (640 x 480) and 1 M records as render_frame gives them (raw, organized): the first call and the best of the repeats.  In
the same run, on the same frame: the repeat of rsreg_cloud_normals(k = 10), the k-NN estimator it stands beside.

    python tools/iinormals_time.py [--sizes 50k,N300,N1M] [--repeats 5] [--smoothing 10] [--out profiles/iinormals_time.jsonl]
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--smoothing", default="10")
    ap.add_argument("--no-knn", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = api.Context(0)
    L = api._l.lib()
    lines = []
    for size in a.sizes.split(","):
        raw = synth.render_frame(1, size)
        dc = api.DeviceCloud(raw, ctx=ctx)
        for s in (float(v) for v in a.smoothing.split(",")):
            prm = api.iin_params(normal_smoothing_size=s)
            out = api.DeviceCloud(ctx=ctx)

            def run():
                api._l.check(L.rsreg_cloud_integral_normals(ctx.h, dc.h, prm, out.h, None), ctx.h)
                ctx.synchronize()
            first, repeat = best(run, a.repeats)
            with_normal = float(np.isfinite(out.download_normals().points["normal_x"]).mean())
            line = {"size": size, "form": "raw", "width": raw.width, "height": raw.height, "records": len(raw), "smoothing": s,
                    "share_with_normal": round(with_normal, 4),
                    "gpu_integral_normals_first_ms": round(first, 3), "gpu_integral_normals_repeat_ms": round(repeat, 3)}
            if not a.no_knn:
                knn_out = api.DeviceCloud(ctx=ctx)

                def run_knn():
                    api._l.check(L.rsreg_cloud_normals(ctx.h, dc.h, 10, None, knn_out.h), ctx.h)
                    ctx.synchronize()
                _, knn_repeat = best(run_knn, a.repeats)
                line.update({"gpu_knn_normals_k10_repeat_ms": round(knn_repeat, 3), "knn_over_integral": round(knn_repeat / repeat, 2)})
                knn_out.close()
            print(json.dumps(line), flush=True)
            lines.append(line)
            out.close()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
