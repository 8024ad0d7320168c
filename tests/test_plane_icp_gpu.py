"""Point-to-plane ICP on the GPU (estimation = RSREG_ESTIMATION_POINT_TO_PLANE_LLS: k_plane_reduce, the 6-unknown solve)
against tests/plane_ref.py.

Step-wise (begin -> search -> plane_sums -> update_plane): the 32 sums against the reference fed the engine's own
(index, d2) within (n_terms + 16) * 2^-53 * sum|term|, sums [0] and [1] bit-equal to the point-to-point sums [0] and [16] of the
same search on a second context, the increment against plane_ref.plane_solve of the same sums (tests/plane_cases.py).
Whole alignments: the 50 k synthetic "bench" pair within 1e-4 (Frobenius) of plane_ref.plane_icp, the pipeline modes, device
clouds, a one-plane target, getFitnessScore, the error paths."""
import os
import subprocess
import sys

import numpy as np
import pytest

import filters_ref
import fitness_ref
import plane_cases as PC
import plane_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = PC.GATE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    return api


@pytest.fixture(scope="module")
def ctxs(api):
    return api.Context(0), api.Context(0)


@pytest.fixture(scope="module")
def walls():
    return PC.three_walls(2000)


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 127, 128, 129, 1000])
def test_sums_and_increment_at_tile_and_wave_edges(api, ctxs, walls, n):
    tgt, nrm = walls
    PC.stepwise_check(api, PC.source_near(tgt, n, seed=100 + n), tgt, nrm, ctx=ctxs[0], ctx2=ctxs[1], label="n=%d" % n)


def test_merged_copies_carry_their_weight(api, ctxs, walls):
    """70 000 source records of which 10 000 are exact copies: above 65 536 records the engine merges copies, W = cur.w."""
    tgt, nrm = walls
    src = PC.source_near(tgt, 60_000, seed=7)
    rng = np.random.default_rng(8)
    src = np.concatenate([src, src[rng.integers(0, 60_000, 10_000)]])
    src = src[rng.permutation(len(src))]
    icp_n = []

    def set_target(icp):
        icp.setInputTarget(PC.cloud(tgt), PC.normal_cloud(api, nrm))
        icp_n.append(icp)
    PC.stepwise_check(api, src, tgt, nrm, ctx=ctxs[0], ctx2=ctxs[1], set_target=set_target, label="70k with copies")
    # (the engine merges the copies its spatial sort brings together, not necessarily all of them: some pairs carry W > 1)
    assert 60_000 <= icp_n[0].grid_info().n_source_distinct < 70_000


def test_scan_path_target_builds_its_index_after_all(api):
    """A device-cloud target set for at most 64 source points is searched whole (index_kind 2); plane mode needs the sorted
    records' original indices and builds the index at begin."""
    tgt, nrm = PC.three_walls(40_000, seed=9)
    src = PC.source_near(tgt, 40, seed=10)
    ctx = api.Context(0)
    dev = api.DeviceCloud(PC.cloud(tgt), ctx=ctx)
    seen = []

    def set_target(icp):
        icp.setInputSource(api.DeviceCloud(PC.cloud(src), ctx=ctx))
        icp._n_src = len(src)
        icp.setInputTarget(dev, PC.normal_cloud(api, nrm))
        icp._sync_inputs()
        seen.append((icp, icp.grid_info().index_kind))
    PC.stepwise_check(api, src, tgt, nrm, ctx=ctx, set_target=set_target, label="scan-path target")
    assert seen[0][1] == 2 and seen[0][0].grid_info().index_kind in (0, 1)


@pytest.mark.parametrize("env,kind", [({"RSREG_FORCE_HASH": "1"}, 0), ({}, 1)], ids=["brick-hash", "dense-grid"])
def test_both_index_kinds(env, kind):
    e = dict(os.environ, PLANE_CASE_INDEX_KIND=str(kind), PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "plane_cases.py"), "walls_index_kind"], cwd=ROOT, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "plane case ok" in r.stdout, r.stdout[-3000:]


def test_non_finite_records_and_points_outside_the_gate(api, ctxs, walls):
    tgt, nrm = walls
    src = PC.source_near(tgt, 500, seed=11)
    src[3] = np.nan
    src[10, 1] = np.inf
    src[77] = (-np.inf, np.nan, 0)
    src[100:160] += np.float32(0.5)        # far outside the 5 cm gate
    sums = PC.stepwise_check(api, src, tgt, nrm, ctx=ctxs[0], ctx2=ctxs[1], label="NaN, Inf, unmatched")
    assert 3 <= sums[0] <= 500 - 3 - 60 + 5


def test_every_third_normal_nan(api, ctxs, walls):
    tgt, nrm = walls
    nrm = nrm.copy()
    nrm[::3, 0] = np.nan                   # (every record of the wall x = -1: that wall drops out of the system)
    nrm[1::30, 2] = np.inf
    sums = PC.stepwise_check(api, PC.source_near(tgt, 1000, seed=12), tgt, nrm, ctx=ctxs[0], ctx2=ctxs[1], label="every third normal NaN")
    assert 0 < sums[2] < sums[0]


def test_normals_from_the_device_from_the_host_and_inside_the_records(api):
    """DeviceCloud.normals(k = 10) through rsreg_icp_set_target_normals_cloud, the same normals downloaded and handed in at
    stride 32, and packed into 48-byte PointXYZRGBNormal records at stride 48: the same 32 doubles, bit for bit."""
    from rsreg_amd import synth
    tgt = filters_ref.xyz(synth.render_frame(0, (80, 60), "bench"))
    src = filters_ref.xyz(synth.render_frame(1, (80, 60), "bench"))
    ctx = api.Context(0)
    dev_tgt = api.DeviceCloud(PC.cloud(tgt), ctx=ctx)
    dev_nrm = dev_tgt.normals_cloud(10)
    host_nrm = dev_nrm.download_normals()
    nrm = np.stack([host_nrm.points[k] for k in ("normal_x", "normal_y", "normal_z")], 1)
    rec48 = np.zeros(len(tgt), api.POINT_NORMAL_DTYPE)
    for k, col in zip(("x", "y", "z"), tgt.T):
        rec48[k] = col
    for k, col in zip(("normal_x", "normal_y", "normal_z"), nrm.T):
        rec48[k] = col
    rec48["curvature"] = host_nrm.points["curvature"]
    got = []
    for how in ("device", "host-32", "records-48"):
        def set_target(icp, how=how):
            if how == "device":
                icp.setInputTarget(PC.cloud(tgt))
                icp.setInputTargetNormals(dev_nrm)
            elif how == "host-32":
                icp.setInputTarget(PC.cloud(tgt), host_nrm)
            else:
                icp.setInputTarget(rec48)
        got.append(PC.stepwise_check(api, src, tgt, nrm, ctx=ctx, set_target=set_target, label=how))
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()
    assert got[0][2] > 100


@pytest.mark.parametrize("params", [dict(use_reciprocal_correspondences=1), dict(trim_overlap_ratio=0.7),
                                    dict(use_reciprocal_correspondences=1, trim_overlap_ratio=0.7)], ids=["reciprocal", "trimmed", "both"])
def test_correspondence_filters(api, ctxs, walls, params):
    """The sums run over the pairs rsreg_icp_search reports as kept (the weighted form of the kernel)."""
    tgt, nrm = walls
    src = PC.source_near(tgt, 1500, seed=13)
    src[1000:] = src[:500]                 # copies: the filters decide per record
    sums = PC.stepwise_check(api, src, tgt, nrm, ctx=ctxs[0], ctx2=ctxs[1], label=str(params), **params)
    assert 3 <= sums[0] < 1500


def _align(api, ctx, src, tgt, nrm, iterations=10, guess=None, **kw):
    icp = api.IterativeClosestPointWithNormals(ctx)
    icp.params = api.icp_params(max_iterations=iterations, criteria_mode=1, max_correspondence_distance=GATE, estimation=1, **kw)
    icp.setInputSource(src)
    icp.setInputTarget(tgt, nrm)
    out = icp.align(guess)
    return icp, out


def test_determinism_across_runs_and_contexts(api, walls):
    tgt, nrm = walls
    src = PC.cloud(PC.source_near(tgt, 3000, seed=14))
    ctx = api.Context(0)
    runs = []
    for _ in range(2):
        icp, _ = _align(api, ctx, src, PC.cloud(tgt), PC.normal_cloud(api, nrm), iterations=4)
        runs.append((bytes(icp.result.transform), icp.plane_sums_last().tobytes(), icp.result.n_correspondences))
    fresh = api.Context(0)
    other, other_n = PC.three_walls(5000, seed=21, extent=2.0)
    _align(api, fresh, PC.cloud(PC.source_near(other, 700, seed=22)), PC.cloud(other), PC.normal_cloud(api, other_n), iterations=2)
    icp, _ = _align(api, fresh, src, PC.cloud(tgt), PC.normal_cloud(api, nrm), iterations=4)
    runs.append((bytes(icp.result.transform), icp.plane_sums_last().tobytes(), icp.result.n_correspondences))
    assert runs[0] == runs[1] == runs[2]
    assert icp.result.iterations == 4 and runs[0][2] > 2000


@pytest.fixture(scope="module")
def bench(api):
    """The 50 k "bench" pair, the target's normals (k = 10, computed once on the device and handed to engine and reference
    alike) and the reference alignment."""
    from rsreg_amd import synth
    tgt = synth.render_frame(0, "50k", "bench")
    src = synth.render_frame(1, "50k", "bench")
    ctx = api.Context(0)
    dev = api.DeviceCloud(tgt, ctx=ctx)
    nrm_dev = dev.normals_cloud(10)
    nrm = nrm_dev.download_normals()
    n3 = np.stack([nrm.points[k] for k in ("normal_x", "normal_y", "normal_z")], 1)
    ref = plane_ref.plane_icp(filters_ref.xyz(src), filters_ref.xyz(tgt), n3, None, 10, GATE, synth.ground_truth(1, 0, "bench"))
    icp, out = _align(api, ctx, src, tgt, nrm, pipeline_mode=0)
    return dict(src=src, tgt=tgt, nrm=nrm, ref=ref, ctx=ctx, icp=icp, out=out, dev_tgt=dev, dev_nrm=nrm_dev)


def test_bench_pair_alignment_matches_the_reference_loop(api, bench):
    icp, ref = bench["icp"], bench["ref"]
    T = icp.getFinalTransformation()
    err = float(np.linalg.norm(T.astype(np.float64) - ref.T.astype(np.float64)))
    print("|T - T_ref|_F = %.3g, n_correspondences %d / %d, |T_ref - truth|_F per iteration %s"
          % (err, icp.result.n_correspondences, ref.n_correspondences, ["%.3g" % e for e in ref.errors]))
    assert err < 1e-4
    assert icp.result.iterations == 10 == ref.iterations and api.CONV_STATES[icp.result.state] == "ITERATIONS"
    assert icp.result.n_correspondences == ref.n_correspondences
    assert icp.result.mse == icp.plane_sums_last()[1] / icp.plane_sums_last()[0]
    # the aligned cloud: the source records at the final pose
    want = api.transformPointCloud(bench["src"], T, ctx=bench["ctx"])
    for k in "xyz":
        np.testing.assert_array_equal(bench["out"].points[k], want.points[k])


@pytest.mark.parametrize("mode", [1, 2], ids=["fused", "device-loop"])
def test_requested_pipeline_modes_fall_back_to_staged(api, bench, mode):
    icp, _ = _align(api, api.Context(0), bench["src"], bench["tgt"], bench["nrm"], pipeline_mode=mode)
    assert bytes(icp.result.transform) == bytes(bench["icp"].result.transform)
    assert icp.plane_sums_last().tobytes() == bench["icp"].plane_sums_last().tobytes()
    assert icp.result.n_nn_launches == 10


def test_device_clouds_give_the_host_result(api, bench):
    ctx = bench["ctx"]
    dev_src = api.DeviceCloud(bench["src"], ctx=ctx)
    icp, out = _align(api, ctx, dev_src, bench["dev_tgt"], bench["dev_nrm"])
    assert bytes(icp.result.transform) == bytes(bench["icp"].result.transform)
    assert icp.result.n_correspondences == bench["icp"].result.n_correspondences
    got = out.download()
    for k in "xyz":
        np.testing.assert_array_equal(got.points[k], bench["out"].points[k])


def test_fitness_score_after_a_plane_alignment(api, bench):
    ctx = bench["ctx"]
    icp, _ = _align(api, ctx, bench["src"], bench["tgt"], bench["nrm"])
    score, count = icp.fitnessScore(GATE * GATE)
    src, tgt = filters_ref.xyz(bench["src"]), filters_ref.xyz(bench["tgt"])
    pos = filters_ref.xyz(api.transformPointCloud(bench["src"], icp.getFinalTransformation(), ctx=ctx))
    want, want_n = fitness_ref.fitness(pos, tgt, GATE * GATE, valid=fitness_ref.finite_rows(src))
    assert count == want_n and abs(score - want) <= 1e-12 * want


def test_one_plane_target_stays_finite_and_orthonormal(api):
    rng = np.random.default_rng(31)
    tgt = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    tgt[:, 2] = 2.0
    nrm = np.zeros_like(tgt)
    nrm[:, 2] = -1.0
    src = tgt[:1500].copy()
    src[:, 2] += np.float32(0.02)
    src[:, 0] += np.float32(0.003)         # (sliding along the plane: the data says nothing about it)
    icp, _ = _align(api, api.Context(0), PC.cloud(src), PC.cloud(tgt), PC.normal_cloud(api, nrm))
    T = icp.getFinalTransformation().astype(np.float64)
    assert np.isfinite(T).all() and icp.result.iterations == 10
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(T[:3, :3]) - 1) < 1e-6
    assert (T[3] == (0, 0, 0, 1)).all()
    assert abs(T[2, 3] + 0.02) < 1e-3 and abs(T[0, 3]) < 1e-3


def test_error_paths(api, walls):
    from rsreg_amd import lib as L
    import ctypes as C
    tgt, nrm = walls
    src = PC.source_near(tgt, 200, seed=41)
    ctx = api.Context(0)
    lib = L.lib()
    t, s, n = PC.cloud(tgt).points, PC.cloud(src).points, PC.normal_cloud(api, nrm).points
    plane = api.icp_params(max_correspondence_distance=GATE, estimation=1)
    point = api.icp_params(max_correspondence_distance=GATE)
    assert lib.rsreg_icp_set_target_normals(ctx.h, n.ctypes.data, len(n), 32) == -5           # RSREG_ERR_NO_TARGET
    assert lib.rsreg_icp_set_source(ctx.h, s.ctypes.data, len(s), 32, 0) == 0
    assert lib.rsreg_icp_set_target(ctx.h, t.ctypes.data, len(t), 32, 0, GATE) == 0
    assert lib.rsreg_icp_begin(ctx.h, None, C.byref(plane)) == L.RSREG_ERR_STATE              # plane mode before the normals
    assert lib.rsreg_icp_set_target_normals(ctx.h, n.ctypes.data, len(n) - 1, 32) == L.RSREG_ERR_INVALID_ARG
    assert lib.rsreg_icp_begin(ctx.h, None, C.byref(plane)) == L.RSREG_ERR_STATE
    assert lib.rsreg_icp_set_target_normals(ctx.h, n.ctypes.data, len(n), 32) == 0
    bad = api.icp_params(max_correspondence_distance=GATE, estimation=2)
    assert lib.rsreg_icp_begin(ctx.h, None, C.byref(bad)) == L.RSREG_ERR_INVALID_ARG
    sums = np.zeros(32)
    done = C.c_int(0)
    assert lib.rsreg_icp_begin(ctx.h, None, C.byref(plane)) == 0
    assert lib.rsreg_icp_plane_sums(ctx.h, sums.ctypes.data) == L.RSREG_ERR_STATE             # before the search
    assert lib.rsreg_icp_search(ctx.h, None, None) == 0
    assert lib.rsreg_icp_sums(ctx.h, sums.ctypes.data) == L.RSREG_ERR_STATE                   # the 17 sums in plane mode
    assert lib.rsreg_icp_update(ctx.h, sums.ctypes.data, None, C.byref(done)) == L.RSREG_ERR_STATE
    assert lib.rsreg_icp_plane_sums(ctx.h, sums.ctypes.data) == 0 and sums[0] >= 3
    assert lib.rsreg_icp_update_plane(ctx.h, sums.ctypes.data, None, C.byref(done)) == 0
    assert lib.rsreg_icp_end(ctx.h, None, None, 0) == 0
    assert lib.rsreg_icp_begin(ctx.h, None, C.byref(point)) == 0                              # and the other way round
    assert lib.rsreg_icp_search(ctx.h, None, None) == 0
    assert lib.rsreg_icp_plane_sums(ctx.h, sums.ctypes.data) == L.RSREG_ERR_STATE
    assert lib.rsreg_icp_update_plane(ctx.h, sums.ctypes.data, None, C.byref(done)) == L.RSREG_ERR_STATE
    s17 = np.zeros(17)
    assert lib.rsreg_icp_sums(ctx.h, s17.ctypes.data) == 0
    assert lib.rsreg_icp_update(ctx.h, s17.ctypes.data, None, C.byref(done)) == 0
    assert lib.rsreg_icp_end(ctx.h, None, None, 0) == 0
    last = np.ones(32)
    assert lib.rsreg_icp_plane_sums_last(ctx.h, last.ctypes.data) == 0 and not last.any()     # all 0 after a point-to-point one
    assert lib.rsreg_icp_set_target(ctx.h, t.ctypes.data, len(t), 32, 0, GATE) == 0           # a second set_target drops the normals
    assert lib.rsreg_icp_begin(ctx.h, None, C.byref(plane)) == L.RSREG_ERR_STATE
    assert lib.rsreg_icp_begin(ctx.h, None, C.byref(point)) == 0
    assert lib.rsreg_icp_end(ctx.h, None, None, 0) == 0
