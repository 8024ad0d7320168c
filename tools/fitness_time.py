"""getFitnessScore after the bench-shaped 1 M <-> 1 M alignment and a 300 k pair: host wall time of rsreg_icp_fitness_score at
DBL_MAX and at the gate (the first call after a target change includes the fitness index's build), NDT's on the 300 k pair, the
extra time rsreg_ndt_set_target spends keeping the target's points, and how many records had to walk beyond the rings the
alignment's index was built for (their nearest target lies farther than the gate: n_within(DBL_MAX) - n_within(gate^2)).

    python tools/fitness_time.py [--reps 20]
Under `rocprofv3 --kernel-trace --stats -- python tools/fitness_time.py` the per-kernel times are k_fit_search / k_fit_tiles /
k_final_reduce (every call) and k_grid_box / k_grid_count / k_oscan_* / k_grid_scatter (the build: pointgrid.hpp).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _ms(f, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = f()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out)), r


def pair(api, synth, size, gate, reps):
    tgt, src = synth.render_frame(0, size, "bench"), synth.render_frame(1, size, "bench")
    guess = synth.small_transform(1.0, (0.008, -0.004, 0.006)).astype(np.float32)
    ctx = api.Context(0)
    icp = api.IterativeClosestPoint(ctx)
    icp.params = api.icp_params(max_correspondence_distance=gate, max_iterations=30, criteria_mode=1, pipeline_mode=2)
    icp.setInputSource(src)
    icp.setInputTarget(tgt)
    icp.align(guess)
    t = time.perf_counter()
    first = icp.fitnessScore()
    first_ms = (time.perf_counter() - t) * 1e3
    full_ms, full = _ms(icp.fitnessScore, reps)
    gate_ms, at_gate = _ms(lambda: icp.fitnessScore(gate * gate), reps)
    res = {"points": [len(src), len(tgt)], "gate": gate, "first_call_ms": first_ms, "dbl_max_ms": full_ms, "at_gate_ms": gate_ms,
           "score": full[0], "n_within": full[1], "score_at_gate": at_gate[0], "n_within_gate": at_gate[1],
           "walked_beyond_gate": full[1] - at_gate[1]}
    if size == "N300":
        ndt = api.NormalDistributionsTransform(ctx)
        ndt.params = api.ndt_params(reference=True)
        ndt.setInputSource(src)
        ndt.setInputTarget(tgt)
        ndt.align(guess)
        t = time.perf_counter()
        nf = ndt.fitnessScore()
        res["ndt_first_call_ms"] = (time.perf_counter() - t) * 1e3
        res["ndt_ms"], _ = _ms(ndt.fitnessScore, reps)
        res["ndt_score"], res["ndt_n_within"] = nf
        # what rsreg_ndt_set_target costs with the points kept (the copy is one launch inside it)
        keep, p, n, s = api._records(tgt)
        from rsreg_amd import lib as L
        res["ndt_set_target_ms"], _ = _ms(lambda: L.check(L.lib().rsreg_ndt_set_target(ctx.h, p, n, s, 0, 1.0), ctx.h), reps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from rsreg_amd import api, synth
    out = {"N1M": pair(api, synth, "N1M", 0.05, a.reps), "N300": pair(api, synth, "N300", 0.01, a.reps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
