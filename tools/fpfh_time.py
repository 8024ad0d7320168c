"""Host wall time of rsreg_cloud_fpfh (k = 10, 20, 50) on rendered frames of 50 k, 307 k and 1 M records: the first call and the
best of the repeats, on the frame after PassThrough(z, 0.2, 2.5) and on the raw frame with its pile of missing-depth records at
the origin.  The normals are rsreg_cloud_normals' at the same k, computed before the clock starts.  Beside it, in the same run on
the same frame: the repeat of rsreg_cloud_normals(k), which holds the same search -- the yardstick.

    python tools/fpfh_time.py [--sizes 50k,N300,N1M] [--repeats 3] [--ks 10,20,50] [--forms passthrough,raw] [--out profiles/fpfh_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rsreg_amd  # noqa: E402,F401
from rsreg_amd import api  # noqa: E402
from rsreg_amd import synth  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_time.jsonl"))
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
            for k in (int(v) for v in a.ks.split(",")):
                normals, out = api.DeviceCloud(ctx=ctx), api.DeviceCloud(ctx=ctx)

                def run_normals():
                    api._l.check(L.rsreg_cloud_normals(ctx.h, dc.h, k, None, normals.h), ctx.h)
                    ctx.synchronize()

                def run_fpfh():
                    api._l.check(L.rsreg_cloud_fpfh(ctx.h, dc.h, normals.h, k, out.h), ctx.h)
                    ctx.synchronize()
                n_first, n_repeat = best(run_normals, a.repeats)
                first, repeat = best(run_fpfh, a.repeats)
                line = {"size": size, "form": form, "records": len(dc), "k": k,
                        "gpu_fpfh_first_ms": round(first, 3), "gpu_fpfh_repeat_ms": round(repeat, 3),
                        "gpu_normals_first_ms": round(n_first, 3), "gpu_normals_repeat_ms": round(n_repeat, 3),
                        "ratio_repeat": round(repeat / n_repeat, 2)}
                print(json.dumps(line), flush=True)
                lines.append(line)
                normals.close()
                out.close()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
