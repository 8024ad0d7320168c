"""SampleConsensusInitialAlignment on the scenario of tools/prerej_time.py: two rendered frames a known LARGE motion apart, VoxelGrid ->
NormalEstimation(10) -> FPFHEstimation(10) -> feature_knn(k) -> initial_alignment (poses from descriptor neighbours, EVERY one scored
over every source record).  Per leaf one line: host wall time of rsreg_cloud_initial_alignment, first call / best repeat, at each
iteration count with the truncated error (thr = (2.5 leaves)^2, min_sample_distance 10 leaves) and with Huber's; and the wall time of
rsreg_cloud_error_transforms over the fixed transforms tools/prerej_time.py scores, beside rsreg_cloud_score_transforms at
max_range = 2.5 leaves over the same transforms IN THE SAME RUN: the same search with the same bound on the same grid (the yardstick
adds a ballot and an atomic, the new kernel a division).  The two are timed alternately, A B A B .., and every repeat is kept, so that
the spread of a call is there beside the difference of the two.  Everything is reported, nothing asserted.

    python tools/scia_time.py [--frames 0,20] [--leaves 0.06,0.03,0.015] [--size N300] [--k 5] [--iterations 1000,4096]
                              [--transforms 4096] [--repeats 3] [--out profiles/scia_time.jsonl]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rsreg_amd  # noqa: E402,F401
from rsreg_amd import api  # noqa: E402
from rsreg_amd import synth  # noqa: E402
from prerej_time import around, best  # noqa: E402


def alternately(calls, repeats):
    """{name: [ms of the warm-up, ms of each repeat ..]}: one warm-up of each, then the calls in turn, `repeats` times"""
    ms = {name: [] for name, _ in calls}
    for _ in range(1 + repeats):
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()                                   # (every call here waits for the stream before it returns)
            ms[name].append(round((time.perf_counter() - t0) * 1e3, 3))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="0,20")
    ap.add_argument("--leaves", default="0.06,0.03,0.015")
    ap.add_argument("--size", default="N300")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--iterations", default="1000,4096")
    ap.add_argument("--transforms", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--range-leaves", type=float, default=2.5, help="thr = (this many leaf sizes)^2")
    ap.add_argument("--sample-leaves", type=float, default=10.0, help="min_sample_distance in leaf sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scia_time.jsonl"))
    a = ap.parse_args()
    ctx = api.Context(0)
    ks, kt = (int(v) for v in a.frames.split(","))
    truth = synth.ground_truth(ks, kt, "bench")
    frames = synth.render_frame(ks, a.size, preset="bench"), synth.render_frame(kt, a.size, preset="bench")

    def err(T):
        return None if T is None else round(float(np.linalg.norm(np.asarray(T, np.float64) - truth)), 6)

    lines = []
    for leaf in (float(v) for v in a.leaves.split(",")):
        src, tgt = (api.DeviceCloud(f, ctx=ctx).voxel_grid(leaf) for f in frames)
        fs, ft = (c.fpfh_cloud(c.normals_cloud(10), 10) for c in (src, tgt))
        nbr, _ = fs.feature_knn(ft, a.k)
        rng_m = a.range_leaves * leaf
        thr = rng_m * rng_m
        rec = {"frames": [ks, kt], "size": a.size, "leaf": leaf, "ns": len(src), "nt": len(tgt), "k": a.k, "eligible": int((nbr[:, 0] >= 0).sum()),
               "max_correspondence_distance": thr, "min_sample_distance": a.sample_leaves * leaf, "runs": []}
        out = {}
        for fn, tag in ((api.SCIA_TRUNCATED, "truncated"), (api.SCIA_HUBER, "huber")):
            for its in (int(v) for v in a.iterations.split(",")):
                prm = dict(max_iterations=its, max_correspondence_distance=thr, min_sample_distance=a.sample_leaves * leaf, error_function=fn, seed=1)

                def run():
                    out["res"] = src.initial_alignment(tgt, nbr, **prm)
                first, repeat = best(run, a.repeats)
                res = out["res"]
                rec["runs"].append({"error_function": tag, "iterations": its, "first_ms": round(first, 3), "repeat_ms": round(repeat, 3), "n_valid": res.n_valid,
                                    "found": res.found, "best_hypothesis": res.best_hypothesis, "error": res.error, "err_initial_alignment": err(res.transform)})
        Ts = around(truth, a.transforms)
        ms = alternately([("score_transforms", lambda: src.score_transforms(tgt, Ts, rng_m)),
                          ("error_transforms_truncated", lambda: src.error_transforms(tgt, Ts, api.SCIA_TRUNCATED, thr)),
                          ("error_transforms_huber", lambda: src.error_transforms(tgt, Ts, api.SCIA_HUBER, thr))], a.repeats)
        rec["transforms"] = a.transforms
        for name, v in ms.items():
            rec[name + "_first_ms"], rec[name + "_repeats_ms"], rec[name + "_repeat_ms"] = v[0], v[1:], min(v[1:])
        rec["truncated_over_score_transforms"] = round(rec["error_transforms_truncated_repeat_ms"] / rec["score_transforms_repeat_ms"], 4)
        rec["huber_over_truncated"] = round(rec["error_transforms_huber_repeat_ms"] / rec["error_transforms_truncated_repeat_ms"], 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        for c in (src, tgt, fs, ft):
            c.close()
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
