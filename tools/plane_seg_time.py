"""Host wall time of the plane segmentation's scoring stage and of whole segmentations: rsreg_cloud_plane_count at n = 307 200 and
n = 1 000 000 records with H = 1 024 and H = 4 096 models, and rsreg_cloud_plane_segment at PCL's defaults and at max_iterations
1 000, warmed, the median of the repeats.  Beside each count, in the same process, rsreg_cloud_count_inliers at the same n and H
(the identity correspondence list over the same cloud, rigid transforms): the kernel the plane count was modelled on, which reads
twice the coordinates and does about three times the arithmetic a test.  Beside both, the issue bound of k_plane_count: its inner
loop is 25 vector instructions a wave for 4 x 64 (record, hypothesis) tests, 12 of them packed-f32 (taken as two passes each, which
is what the chip's f32 vector peak implies), i.e. 37 passes of 2 cycles on one of 256 x 4 SIMDs at 2.4 GHz.  One JSON line per
measurement; what profiles/plane_seg_time.jsonl holds.

    python tools/plane_seg_time.py [--sizes 307200,1000000] [--models 1024,4096] [--repeats 9] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rsreg_amd  # noqa: E402,F401
from rsreg_amd import PointCloud, api  # noqa: E402

SIMDS, CLOCK_HZ = 256 * 4, 2.4e9                      # MI355X: 256 CUs of 4 SIMDs, 2.4 GHz at most
PASSES_PER_WAVE_HYPOTHESIS, TESTS_PER_WAVE_HYPOTHESIS, CYCLES_PER_PASS = 37, 4 * 64, 2


def issue_bound_ms(n, H):
    return n * H / TESTS_PER_WAVE_HYPOTHESIS * PASSES_PER_WAVE_HYPOTHESIS * CYCLES_PER_PASS / (SIMDS * CLOCK_HZ) * 1e3


def timed(call, repeats):
    call()                                             # warm: buffers grown, code loaded
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def scene(n, seed=0):
    """a floor (half the records, sigma 2 mm), a wall (a quarter) and clutter in a 4 m room"""
    rng = np.random.default_rng(seed)
    nf, nw = n // 2, n // 4
    floor = np.stack([rng.uniform(0, 4, nf), rng.uniform(0, 4, nf), rng.normal(0, 0.002, nf)], axis=1)
    wall = np.stack([rng.normal(0, 0.002, nw), rng.uniform(0, 4, nw), rng.uniform(0, 2.5, nw)], axis=1)
    clutter = rng.uniform(0, [4, 4, 2.5], (n - nf - nw, 3))
    return np.ascontiguousarray(np.concatenate([floor, wall, clutter])[rng.permutation(n)], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="307200,1000000")
    ap.add_argument("--models", default="1024,4096")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = api._l.lib()
    ctx = api.Context(0)
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    rng = np.random.default_rng(1)
    for n in (int(s) for s in a.sizes.split(",")):
        dc = api.DeviceCloud(PointCloud.from_xyz(scene(n)), ctx=ctx)
        corr = np.zeros(n, api.CORRESPONDENCE_DTYPE)
        corr["index_query"] = corr["index_match"] = np.arange(n)
        for H in (int(s) for s in a.models.split(",")):
            nrm = rng.normal(size=(H, 3))
            nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            models = np.ascontiguousarray(np.concatenate([nrm, rng.uniform(-2, 0, (H, 1))], axis=1), np.float32)
            counts = np.zeros(H, np.uint32)
            T = np.tile(np.eye(4, dtype=np.float32), (H, 1, 1))
            T[:, :3, 3] = rng.normal(0, 0.01, (H, 3))
            packed = np.ascontiguousarray(T.transpose(0, 2, 1))

            def plane():
                api._l.check(L.rsreg_cloud_plane_count(ctx.h, dc.h, models.ctypes.data, H, 0.01, counts.ctypes.data), ctx.h)

            def pairs():
                api._l.check(L.rsreg_cloud_count_inliers(ctx.h, dc.h, dc.h, corr.ctypes.data, n, packed.ctypes.data, H, 0.02, counts.ctypes.data), ctx.h)

            p_med, p_min = timed(plane, a.repeats)
            c_med, c_min = timed(pairs, a.repeats)
            bound = issue_bound_ms(n, H)
            emit({"what": "plane_count", "records": n, "models": H, "plane_count_median_ms": round(p_med, 3), "plane_count_min_ms": round(p_min, 3),
                  "count_inliers_median_ms": round(c_med, 3), "count_inliers_min_ms": round(c_min, 3), "ratio_median": round(p_med / c_med, 3),
                  "issue_bound_ms": round(bound, 4), "fraction_of_issue_bound": round(bound / p_med, 3)})
        for max_it in (50, 1000):
            res = [None]

            def segment():
                res[0] = dc.segment_plane(capacity=0, distance_threshold=0.01, max_iterations=max_it)[2]

            s_med, s_min = timed(segment, a.repeats)
            r = res[0]
            emit({"what": "plane_segment", "records": n, "max_iterations": max_it, "segment_median_ms": round(s_med, 3), "segment_min_ms": round(s_min, 3),
                  "found": int(r.found), "iterations": r.iterations, "skipped": r.skipped, "inliers": r.n_inliers, "refined": int(r.refined)})
        dc.close()


if __name__ == "__main__":
    main()
