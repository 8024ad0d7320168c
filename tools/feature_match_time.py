"""Host wall time of feature matching in FPFH space: rsreg_cloud_feature_knn at k = 1, 2, 10 and both correspondence calls, the first
call and the best of the repeats, on descriptors computed on the device (VoxelGrid -> NormalEstimation(10) -> FPFHEstimation(10)) from
two rendered 1 M frames at leaves that leave roughly 5 k, 30 k and 100 k rows -- the sizes at which descriptors are matched -- and one
line on the two raw 307 k frames, the cost of not downsampling.  Beside each, in the same run: cKDTree(target).query(source, k,
workers = 16) in 33-D on the same rows (its build apart; above --tree-sample source rows a sample is queried and the time scaled to
all of them, which the line says), and the issue bound of the brute force, ns * nt * 98 float operations over 256 CUs x 128 lanes x
2.4 GHz, with the fraction of it the repeat reaches.

    python tools/feature_match_time.py [--leaves 0.058,0.026,0.0155] [--raw N300] [--repeats 3] [--ks 1,2,10] [--out profiles/feature_match_time.jsonl]
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
from rsreg_amd import api  # noqa: E402
from rsreg_amd import synth  # noqa: E402

PEAK_FLOPS = 256 * 128 * 2.4e9    # 256 CUs x 128 fp32 lanes x 2.4 GHz, one operation a lane a clock (no FMA: the contract has none)
PAIR_FLOPS = 98                   # 33 subtractions, 33 multiplications, 32 additions


def best(fn, repeats):
    ms = []
    for _ in range(1 + repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[0], min(ms[1:])


def descriptors(ctx, frame, leaf):
    """The frame's FPFH rows at k = 10 in HBM, after VoxelGrid(leaf) if a leaf is given"""
    dc = api.DeviceCloud(frame, ctx=ctx)
    if leaf:
        dc = dc.voxel_grid(leaf)
    return dc.fpfh_cloud(dc.normals_cloud(10), 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", default="0.058,0.026,0.0155")
    ap.add_argument("--frame", default="N1M")
    ap.add_argument("--raw", default="N300")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ks", default="1,2,10")
    ap.add_argument("--tree-sample", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_match_time.jsonl"))
    a = ap.parse_args()
    from scipy.spatial import cKDTree
    ctx = api.Context(0)
    L = api._l.lib()
    ks = [int(v) for v in a.ks.split(",")]
    jobs = [(a.frame, float(v)) for v in a.leaves.split(",") if v] + ([(a.raw, 0.0)] if a.raw else [])
    frames = {}
    lines = []
    for size, leaf in jobs:
        if size not in frames:
            frames[size] = (synth.render_frame(0, size, preset="bench"), synth.render_frame(4, size, preset="bench"))
        src, tgt = descriptors(ctx, frames[size][0], leaf), descriptors(ctx, frames[size][1], leaf)
        ns, nt = len(src), len(tgt)
        bound_ms = ns * nt * PAIR_FLOPS / PEAK_FLOPS * 1e3
        srows, trows = src.download_fpfh().points["histogram"], tgt.download_fpfh().points["histogram"]
        sv, tv = np.isfinite(srows).all(axis=1), np.isfinite(trows).all(axis=1)
        t0 = time.perf_counter()
        tree = cKDTree(trows[tv])
        tree_build_ms = (time.perf_counter() - t0) * 1e3
        sample = srows[sv][:a.tree_sample]
        scale = float(sv.sum()) / max(1, len(sample))
        repeats = a.repeats if leaf else 1
        idx, d2 = np.zeros((ns, max(ks)), np.int32), np.zeros((ns, max(ks)), np.float32)
        out, found = np.zeros(ns, api.CORRESPONDENCE_DTYPE), api.C.c_size_t(0)

        def line(call, first, repeat, **more):
            rec = {"frame": size, "leaf": leaf, "ns": ns, "nt": nt, "valid_ns": int(sv.sum()), "valid_nt": int(tv.sum()), "call": call,
                   "gpu_first_ms": round(first, 3), "gpu_repeat_ms": round(repeat, 3), "issue_bound_ms": round(bound_ms, 4),
                   "fraction_of_issue_bound": round(bound_ms / repeat, 4)}
            rec.update(more)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        for k in ks:
            def run_knn():
                api._l.check(L.rsreg_cloud_feature_knn(ctx.h, src.h, tgt.h, k, idx.ctypes.data, d2.ctypes.data), ctx.h)
            first, repeat = best(run_knn, repeats)
            t0 = time.perf_counter()
            tree.query(sample, k, workers=16)
            tree_ms = (time.perf_counter() - t0) * 1e3
            line("feature_knn", first, repeat, k=k, ckdtree_build_ms=round(tree_build_ms, 1), ckdtree_query_ms=round(tree_ms * scale, 1),
                 ckdtree_rows_queried=len(sample), ckdtree_scaled=bool(scale > 1.0))
        for reciprocal in (0, 1):
            def run_corr():
                api._l.check(L.rsreg_cloud_feature_correspondences(ctx.h, src.h, tgt.h, sys.float_info.max, reciprocal, out.ctypes.data, ns,
                                                                   api.C.byref(found)), ctx.h)
            first, repeat = best(run_corr, repeats)
            # the reciprocal call holds two searches: its bound is twice the forward one's
            line("reciprocal_correspondences" if reciprocal else "correspondences", first, repeat, found=int(found.value),
                 searches=1 + reciprocal, fraction_of_issue_bound=round((1 + reciprocal) * bound_ms / repeat, 4))
        src.close()
        tgt.close()
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
