"""Host wall time of rsreg_cloud_fpfh_radius (FPFHEstimationOMP::setRadiusSearch) at r = 0.01, 0.03 and 0.1 on rendered frames of
50 k, 307 k and 1 M records: the first call and the best of the repeats, on the frame after PassThrough(z, 0.2, 2.5) and on the raw
frame, whose pile of missing-depth records at the origin is the expensive case (every record of the pile reads the whole pile, twice;
nothing is approximated).  The normals are rsreg_cloud_normals(k = 10) of the same frame.  In the same run, on the same frame:
  1. the repeat of rsreg_cloud_normals_radius at the same radius -- it holds the same walk once, the new call holds it twice and
     the pair features: the ratio says where the time goes;
  2. the repeat of rsreg_cloud_fpfh(k = 10);
  3. a CPU figure: cKDTree.query_ball_point (the tree over the whole frame) and the numpy arithmetic of tests/fpfh_radius_ref.py --
     pair features, bins and counts, then the weighting over the SPFH table the GPU left -- on a sample of --cpu-sample finite
     records, scaled to the frame by records / sample.

    python tools/fpfh_radius_time.py [--sizes 50k,N300,N1M] [--repeats 3] [--radii 0.01,0.03,0.1] [--forms passthrough,raw]
                                     [--cpu-sample 2000] [--out profiles/fpfh_radius_time.jsonl]
    python tools/fpfh_radius_time.py --only N300,passthrough,0.03     one case, three calls and nothing else: what a profiler wraps
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rsreg_amd  # noqa: E402,F401
from rsreg_amd import api, synth  # noqa: E402


def best(fn, repeats):
    ms = []
    for _ in range(1 + repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[0], min(ms[1:])


def cpu_sample(xyz, nrm, radius, spfh, sample, chunk=64, seed=0):
    """(tree build ms, query ms, SPFH pass ms, weighting pass ms, pairs) for `sample` finite records of the frame"""
    import fpfh_ref as F
    from fitness_ref import d2_f32
    from radius_ref import r2_f32
    from scipy.spatial import cKDTree
    fin = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    t = xyz[fin]
    t0 = time.perf_counter()
    tree = cKDTree(t.astype(np.float64))
    build = time.perf_counter() - t0
    rows = np.random.default_rng(seed).choice(len(fin), min(sample, len(fin)), replace=False)
    r2 = r2_f32(radius)
    query = first = second = 0.0
    pairs = 0
    for s in range(0, len(rows), chunk):
        part = rows[s:s + chunk]
        t0 = time.perf_counter()
        cand = tree.query_ball_point(t[part].astype(np.float64), radius * (1 + 1e-5), workers=16)
        query += time.perf_counter() - t0
        t0 = time.perf_counter()
        lens = np.fromiter((len(c) for c in cand), np.int64, len(cand))
        J = np.concatenate([np.asarray(c, np.int64) for c in cand])
        I = np.repeat(part, lens)
        d2 = d2_f32(t[I], t[J])
        keep = d2 < r2
        I, J, d2 = fin[I[keep]], fin[J[keep]], d2[keep]
        scaled, valid = F.pair_features(xyz[I], nrm[I], xyz[J], nrm[J])
        valid &= I != J
        local = np.repeat(np.arange(len(part)), lens)[keep]
        b = F.bins_of(scaled) + np.arange(3) * F.BINS
        np.bincount((local[:, None] * F.ROW + b)[valid].reshape(-1), minlength=len(part) * F.ROW)
        first += time.perf_counter() - t0
        t0 = time.perf_counter()
        use = d2 != 0
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            w = np.float32(1.0) / d2[use]
            val = (spfh[J[use]] * w[:, None]).astype(np.float64)
        H = np.zeros((len(part), F.ROW))
        np.add.at(H, local[use], val)
        second += time.perf_counter() - t0
        pairs += len(I)
    return build * 1e3, query * 1e3, first * 1e3, second * 1e3, pairs, len(rows)


def frame_forms(ctx, size):
    raw = synth.render_frame(1, size)
    d_raw = api.DeviceCloud(raw, ctx=ctx)
    p = api.PassThrough()
    p.setInputCloud(d_raw)
    p.setFilterFieldName("z")
    p.setFilterLimits(0.2, 2.5)
    return {"passthrough": p.filter(), "raw": d_raw}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50k,N300,N1M")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--radii", default="0.01,0.03,0.1")
    ap.add_argument("--forms", default="passthrough,raw")
    ap.add_argument("--cpu-sample", type=int, default=2000)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_radius_time.jsonl"))
    a = ap.parse_args()
    ctx = api.Context(0)
    L = api._l.lib()
    if a.only:
        size, form, radius = a.only.split(",")
        dc = frame_forms(ctx, size)[form]
        nd = dc.normals_cloud(10)
        for _ in range(3):
            dc.fpfh_radius_cloud(nd, float(radius)).close()
        return
    lines = []
    for size in a.sizes.split(","):
        forms = frame_forms(ctx, size)
        for form in a.forms.split(","):
            dc = forms[form]
            nd = dc.normals_cloud(10)
            p = dc.download().points
            xyz = np.stack([p["x"], p["y"], p["z"]], axis=1).astype(np.float32)
            nrec = nd.download_normals().points
            nrm = np.stack([nrec["normal_x"], nrec["normal_y"], nrec["normal_z"]], axis=1)
            out = api.DeviceCloud(ctx=ctx)

            def run_k10():
                api._l.check(L.rsreg_cloud_fpfh(ctx.h, dc.h, nd.h, 10, out.h), ctx.h)
            _, k10 = best(run_k10, a.repeats)
            for radius in (float(v) for v in a.radii.split(",")):
                def run_fpfh():
                    api._l.check(L.rsreg_cloud_fpfh_radius(ctx.h, dc.h, nd.h, radius, out.h), ctx.h)

                def run_normals():
                    api._l.check(L.rsreg_cloud_normals_radius(ctx.h, dc.h, radius, None, out.h), ctx.h)
                    ctx.synchronize()
                f_first, f_repeat = best(run_fpfh, a.repeats)
                hist = out.download_fpfh().points["histogram"]
                _, n_repeat = best(run_normals, a.repeats)
                t0 = time.perf_counter()
                spfh, m = dc.spfh_radius(nd, radius, counts=True)
                spfh_ms = (time.perf_counter() - t0) * 1e3
                line = {"size": size, "form": form, "records": len(dc), "radius": radius, "neighbours_max": int(m.max()),
                        "neighbours_mean": round(float(m[m > 0].mean()), 2), "nan_rows": int(np.isnan(hist).any(axis=1).sum()),
                        "gpu_fpfh_radius_first_ms": round(f_first, 3), "gpu_fpfh_radius_repeat_ms": round(f_repeat, 3),
                        "gpu_spfh_radius_with_copy_home_ms": round(spfh_ms, 3),
                        "gpu_normals_radius_repeat_ms": round(n_repeat, 3), "ratio_to_normals_radius": round(f_repeat / n_repeat, 2),
                        "gpu_fpfh_k10_repeat_ms": round(k10, 3)}
                if a.cpu_sample:
                    build, query, first, second, pairs, rows = cpu_sample(xyz, nrm, radius, spfh, a.cpu_sample)
                    scale = int((m > 0).sum()) / max(rows, 1)
                    line.update({"cpu_sample": rows, "cpu_sample_pairs": pairs, "cpu_ckdtree_build_ms": round(build, 1),
                                 "cpu_sample_query_ball_point_ms": round(query, 1), "cpu_sample_spfh_ms": round(first, 1),
                                 "cpu_sample_weighting_ms": round(second, 1),
                                 "cpu_scaled_to_frame_ms": round(build + (query + first + second) * scale, 1)})
                print(json.dumps(line), flush=True)
                lines.append(line)
            out.close()
            nd.close()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
