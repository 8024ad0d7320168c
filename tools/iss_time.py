"""Host wall time of rsreg_cloud_iss_keypoints (pcl::ISSKeypoint3D) at salient / non-max radius 0.06 / 0.04 -- 6 / 4 leaves at leaf
0.01 -- on rendered frames of 50 k, 307 k and 1 M records: the first call and the best of the repeats, on the frame after
PassThrough(z, 0.2, 2.5) and on the raw frame (its pile of missing-depth records at the origin: every record of the pile reads the
whole pile, twice).  In the same run, on the same frame:
  * the repeats of the two calls it stands beside, rsreg_cloud_normals_radius(salient) and rsreg_cloud_radius_count(non_max) -- their
    sum holds both walks, an eigen-solve and one index build MORE than the keypoint call makes, which adds the saliency gather and
    the compaction: the target is at most 1.25 times that sum (reported, not asserted);
  * the repeat of rsreg_cloud_iss_saliency without any output copied home (the index and the first walk alone): what is left of the
    keypoint call is the second walk with its gather of saliencies, and the compaction;
  * what a user would otherwise run on the CPU: cKDTree over the frame, then on 2 000 sampled records query_ball_point at both
    radii, the scatter and numpy.linalg.eigvalsh -- the time of the sample scaled to the frame (the suppression's own compare is
    not in it: it needs the saliency of every neighbour).

    python tools/iss_time.py [--sizes 50k,N300,N1M] [--repeats 3] [--forms passthrough,raw] [--out profiles/iss_time.jsonl]
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

SAMPLE = 2000


def cpu_reference(xyz, salient, non_max):
    """(tree build ms, the sample's ms scaled to the frame)"""
    from scipy.spatial import cKDTree
    t = xyz[np.isfinite(xyz).all(axis=1)].astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(t)
    t1 = time.perf_counter()
    pick = np.random.default_rng(0).choice(len(t), min(SAMPLE, len(t)), replace=False)
    near = tree.query_ball_point(t[pick], salient, workers=16)
    eig = np.zeros((len(pick), 3))
    for k, idx in enumerate(near):
        d = t[idx] - t[pick[k]]
        eig[k] = np.linalg.eigvalsh(d.T @ d)
    tree.query_ball_point(t[pick], non_max, return_length=True, workers=16)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3 * len(t) / len(pick)


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
    ap.add_argument("--salient", type=float, default=0.06)
    ap.add_argument("--non-max", type=float, default=0.04)
    ap.add_argument("--forms", default="passthrough,raw")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iss_time.jsonl"))
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    ctx = api.Context(0)
    L = api._l.lib()
    params = api.iss_params(salient_radius=a.salient, non_max_radius=a.non_max)
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
            n = len(dc)
            out, normals = api.DeviceCloud(ctx=ctx), api.DeviceCloud(ctx=ctx)
            idx, counts, found = np.zeros(n, np.int32), np.zeros(n, np.uint32), C.c_uint64(0)

            def run_keypoints():
                api._l.check(L.rsreg_cloud_iss_keypoints(ctx.h, dc.h, C.byref(params), out.h, idx.ctypes.data, n, C.byref(found)), ctx.h)
                ctx.synchronize()

            def run_saliency():
                api._l.check(L.rsreg_cloud_iss_saliency(ctx.h, dc.h, C.byref(params), None, None, None), ctx.h)

            def run_normals():
                api._l.check(L.rsreg_cloud_normals_radius(ctx.h, dc.h, a.salient, None, normals.h), ctx.h)
                ctx.synchronize()

            def run_count():
                api._l.check(L.rsreg_cloud_radius_count(ctx.h, dc.h, a.non_max, counts.ctypes.data), ctx.h)
            k_first, k_repeat = best(run_keypoints, a.repeats)
            _, s_repeat = best(run_saliency, a.repeats)
            _, n_repeat = best(run_normals, a.repeats)
            _, c_repeat = best(run_count, a.repeats)
            _, k_again = best(run_keypoints, a.repeats)       # (once more behind the others: the spread of the same call)
            m_s = dc.iss_saliency(salient_radius=a.salient, non_max_radius=a.non_max)[2]
            line = {"size": size, "form": form, "records": n, "salient_radius": a.salient, "non_max_radius": a.non_max, "keypoints": int(found.value),
                    "salient_neighbours_max": int(m_s.max()), "salient_neighbours_mean": round(float(m_s[m_s > 0].mean()), 2),
                    "non_max_neighbours_mean": round(float(counts[counts > 0].mean()), 2),
                    "gpu_iss_keypoints_first_ms": round(k_first, 3), "gpu_iss_keypoints_repeat_ms": round(k_repeat, 3),
                    "gpu_iss_keypoints_repeat_again_ms": round(k_again, 3), "gpu_iss_saliency_no_copy_repeat_ms": round(s_repeat, 3),
                    "gpu_normals_radius_salient_repeat_ms": round(n_repeat, 3), "gpu_radius_count_non_max_repeat_ms": round(c_repeat, 3),
                    "ratio_to_the_two_calls": round(min(k_repeat, k_again) / (n_repeat + c_repeat), 3)}
            if not a.no_cpu:
                build, scaled = cpu_reference(dc.download().xyz, a.salient, a.non_max)
                line.update({"cpu_ckdtree_build_ms": round(build, 1), "cpu_sample": SAMPLE, "cpu_eigvalsh_reference_scaled_ms": round(scaled, 1)})
            print(json.dumps(line), flush=True)
            lines.append(line)
            out.close()
            normals.close()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
