"""Host wall time of rsreg_cloud_voxel_grid (pcl::VoxelGrid, exact: one centroid per occupied leaf) on rendered frames of 50 k,
307 k and 1 M records, raw and after PassThrough(z, 0.2, 2.5), at leaves of 0.01, 0.05 and 1.0: the first call and the best of
the repeats.  Beside it, in the same run on the same frame and leaf: the repeat of rsreg_cloud_filter (ApproximateVoxelGrid:
the same stages apart from the box pass and a wider sort -- the yardstick), and a numpy downsample on the CPU (np.unique over
the leaf coordinates, np.bincount for the means of x, y, z: what a user without the engine would write; float64 sums, no
colour).

    python tools/voxelgrid_time.py [--sizes 50k,N300,N1M] [--leaves 0.01,0.05,1.0] [--repeats 5] [--out profiles/voxelgrid_time.jsonl]
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


def cpu_unique(xyz, leaf):
    t0 = time.perf_counter()
    xyz = xyz[np.isfinite(xyz).all(axis=1)]
    ijk = np.floor(xyz * np.float32(1.0 / leaf)).astype(np.int64)
    ijk -= ijk.min(axis=0)
    dims = ijk.max(axis=0) + 1
    key = (ijk[:, 2] * dims[1] + ijk[:, 1]) * dims[0] + ijk[:, 0]
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    cent = np.stack([np.bincount(inv, xyz[:, a], len(cnt)) / cnt for a in range(3)], axis=1)
    return (time.perf_counter() - t0) * 1e3, len(cent)


def best(fn, repeats):
    ms = []
    for _ in range(1 + repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[0], min(ms[1:]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50k,N300,N1M")
    ap.add_argument("--leaves", default="0.01,0.05,1.0")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxelgrid_time.jsonl"))
    a = ap.parse_args()
    ctx = api.Context(0)
    rows = []
    for size in a.sizes.split(","):
        raw = synth.render_frame(1, size)
        d_raw = api.DeviceCloud(raw, ctx=ctx)
        p = api.PassThrough()
        p.setInputCloud(d_raw)
        p.setFilterFieldName("z")
        p.setFilterLimits(0.2, 2.5)
        d_pass = p.filter()
        for form, dc in (("passthrough", d_pass), ("raw", d_raw)):
            xyz = dc.download().xyz
            for leaf in [float(v) for v in a.leaves.split(",")]:
                vg = api.VoxelGrid()
                vg.setLeafSize(leaf)
                vg.setInputCloud(dc)
                first, repeat, out = best(vg.filter, a.repeats)
                av = api.ApproximateVoxelGrid()
                av.setLeafSize(leaf, leaf, leaf)
                av.setInputCloud(dc)
                a_first, a_repeat, a_out = best(av.filter, a.repeats)
                cpu_ms, cpu_leaves = cpu_unique(xyz, leaf)
                row = {"size": size, "form": form, "records": len(dc), "leaf": leaf, "leaves": len(out), "div_b": vg.getNrDivisions().tolist(),
                       "voxelgrid_first_ms": round(first, 3), "voxelgrid_repeat_ms": round(repeat, 3),
                       "approx_first_ms": round(a_first, 3), "approx_repeat_ms": round(a_repeat, 3), "approx_records": len(a_out),
                       "ratio_to_approx": round(repeat / a_repeat, 2), "cpu_unique_ms": round(cpu_ms, 1), "cpu_unique_leaves": cpu_leaves}
                rows.append(row)
                print(json.dumps(row), flush=True)
                out.close()
                a_out.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
