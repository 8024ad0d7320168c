"""Registration::getFitnessScore on the GPU (rsreg_icp_fitness_score / _sums, rsreg_ndt_fitness_score, the Python and C++
adaptors) against tests/fitness_ref.py.

On the H = 2^-10 lattice of tests/test_filter_ties.py, shifted 1 m away from its target so that no record has a
correspondence inside the 1 cm gate (the alignment stops at once and the final transform is the identity), every d2 and every
partial sum is exact: the score must be bit-equal and the count exact -- with every record's neighbour many rings beyond the
index the alignment built, and many of them outside the target's box.  On clouds that do align the score must agree to 1e-12."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fitness_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 2.0 ** -10
GATE = 0.01
DBL_MAX = sys.float_info.max

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    return api


def _cloud(xyz):
    from rsreg_amd import POINT_DTYPE, PointCloud
    pts = np.zeros(len(xyz), POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["w"] = 1.0
    return PointCloud(pts, width=len(xyz), height=1, is_dense=False)


def far_lattice(n, seed=5):
    """(source, target) float32: the target lattice of test_filter_ties (spacing 8 H), the source a lattice record set with exact
    copies, NaN and inf, moved by 1024 H along x, plus records 1e3 and 1e4 m away (exact multiples of H)."""
    from test_filter_ties import lattice_pair
    src, tgt, _, _ = lattice_pair(n, seed)
    src = src.copy()
    src[:, 0] += np.float32(1024 * H)
    far = np.array([[1000.0, 0, 0], [-1000.0, 500.0, 0], [0, 0, 10000.0], [-8192.0, -8192.0, 4096.0]], np.float32)
    src[1:1 + len(far)] = far
    return src, tgt


def _align(api, ctx, src, tgt, gate=GATE, **kw):
    icp = api.IterativeClosestPoint(ctx)
    icp.params = api.icp_params(reference=True, max_correspondence_distance=gate, **kw)
    icp.setInputSource(src if not isinstance(src, np.ndarray) else _cloud(src))
    icp.setInputTarget(tgt if not isinstance(tgt, np.ndarray) else _cloud(tgt))
    icp.align()
    return icp


def _expected(api, ctx, src, tgt, T, max_range=DBL_MAX):
    """The reference score from rsreg_transform_cloud's positions of the source records at T."""
    pos = _xyz(api.transformPointCloud(_cloud(src), T, ctx=ctx))
    return F.fitness(pos, tgt, max_range, valid=F.finite_rows(src))


def _xyz(pc):
    p = pc.points
    return np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float32)


RANGES = [DBL_MAX, 0.9, 0.5, 2.0, 1e8, 0.0, -1.0]


def _lattice_results(api, ctx, src, tgt):
    icp = _align(api, ctx, src, tgt)
    assert icp.result.n_correspondences == 0
    np.testing.assert_array_equal(icp.getFinalTransformation(), np.eye(4, dtype=np.float32))
    return {repr(r): icp.fitnessScore(r) for r in RANGES}


@pytest.mark.parametrize("n", [50_000, 70_001])
def test_lattice_far_from_its_target_is_bit_equal(api, n):
    """Default DBL_MAX range on a target indexed for a 1 cm gate, sources far outside the target's box, a max_range between d and
    d^2, ranges with nothing in them; 50 000 records (plain source load) and 70 001 (sorted, exact copies merged)."""
    src, tgt = far_lattice(n)
    ctx = api.Context(0)
    got = _lattice_results(api, ctx, src, tgt)
    pos = src.copy()
    valid = F.finite_rows(src)
    d = F.nearest_d2(pos, tgt)
    dd = np.sqrt(d[valid].astype(np.float64))
    # 0.9 tells the squared comparison from the unsquared one on this cloud
    assert (d[valid] <= 0.9).sum() != (dd <= 0.9).sum()
    for r in RANGES:
        want = F.fitness(pos, tgt, r, valid=valid)
        assert got[repr(r)][1] == want[1], (r, got[repr(r)], want)
        assert got[repr(r)][0] == want[0], (r, got[repr(r)], want)
    assert got[repr(-1.0)] == (DBL_MAX, 0) and got[repr(0.0)] == (DBL_MAX, 0)
    assert got[repr(DBL_MAX)][1] == int(valid.sum())


_CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from rsreg_amd import api
import test_fitness_score_gpu as T
out = {}
for n in (50000, 70001):
    src, tgt = T.far_lattice(n)
    ctx = api.Context(0)
    res = T._lattice_results(api, ctx, src, tgt)
    out[str(n)] = {k: [v[0].hex(), v[1]] for k, v in res.items()}
print("RESULT " + json.dumps(out))
'''


def _child(env):
    e = dict(os.environ)
    e.update(env)
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


@pytest.fixture(scope="module")
def lattice_default():
    return _child({})


@pytest.mark.parametrize("env", [{"RSREG_FORCE_HASH": "1"}, {"RSREG_NO_NBR_FROM_TABLE": "1"},
                                 {"RSREG_COUNT_SORT": "0", "RSREG_FULL_TABLE": "1"}, {"RSREG_SORT_SMALL": "1"}],
                         ids=["brick-hash", "dense-occupancy-words", "dense-sorted-build-full-table", "sort-small-sources"])
def test_every_index_form_and_source_path_gives_the_same_bits(lattice_default, env):
    assert _child(env) == lattice_default


def test_index_less_target_of_a_small_source(api):
    """A device-cloud target set for <= 64 source points is not indexed at all (grid.dense == 2): the score is still exact."""
    src, tgt = far_lattice(50_000)
    src = src[:64]
    ctx = api.Context(0)
    ds, dt = api.DeviceCloud(_cloud(src), ctx=ctx), api.DeviceCloud(_cloud(tgt), ctx=ctx)
    icp = _align(api, ctx, ds, dt)
    assert icp.grid_info().index_kind == 2
    np.testing.assert_array_equal(icp.getFinalTransformation(), np.eye(4, dtype=np.float32))
    for r in (DBL_MAX, 0.9):
        assert icp.fitnessScore(r) == F.fitness(src, tgt, r, valid=F.finite_rows(src))


@pytest.fixture(scope="module")
def frames():
    from rsreg_amd import synth
    tgt = synth.render_frame(0, "50k", "parity")
    src = synth.render_frame(1, "50k", "parity")
    return src, tgt


def _check_close(got, want):
    assert got[1] == want[1], (got, want)
    assert abs(got[0] - want[0]) <= 1e-12 * abs(want[0]), (got, want)


def test_pipelines_and_filters(api, frames):
    """Staged, fused and device-loop alignments and the correspondence filters: each score agrees with the reference at its own
    final transform; equal transforms give equal bits."""
    src, tgt = frames
    seen = {}
    for kw in [dict(pipeline_mode=0), dict(pipeline_mode=1), dict(pipeline_mode=2), dict(pipeline_mode=2, criteria_mode=1),
               dict(use_reciprocal_correspondences=1), dict(trim_overlap_ratio=0.8)]:
        ctx = api.Context(0)
        icp = _align(api, ctx, src, tgt, gate=0.05, **kw)
        T = icp.getFinalTransformation()
        got = icp.fitnessScore()
        _check_close(got, _expected(api, ctx, F_xyz(src), F_xyz(tgt), T))
        _check_close(icp.fitnessScore(1e-4), _expected(api, ctx, F_xyz(src), F_xyz(tgt), T, 1e-4))
        key = T.tobytes()
        if key in seen:
            assert seen[key] == got
        seen[key] = got


def F_xyz(pc):
    return _xyz(pc) if not isinstance(pc, np.ndarray) else pc


def test_host_records_and_device_cloud_alignments(api, frames):
    src, tgt = frames
    out = []
    for mode in ("records", "host", "device"):
        ctx = api.Context(0)
        if mode == "records":
            icp = _align(api, ctx, src, tgt, gate=0.05)
        elif mode == "host":   # an (n, 4) float32 array: rsreg_icp_align
            a = np.ascontiguousarray(np.stack([_xyz(src)[:, 0], _xyz(src)[:, 1], _xyz(src)[:, 2], np.ones(len(src.points), np.float32)], 1))
            icp = _align(api, ctx, a, tgt, gate=0.05)
        else:
            icp = _align(api, ctx, api.DeviceCloud(src, ctx=ctx), api.DeviceCloud(tgt, ctx=ctx), gate=0.05)
        T = icp.getFinalTransformation()
        got = icp.fitnessScore()
        _check_close(got, _expected(api, ctx, _xyz(src), _xyz(tgt), T))
        out.append((T.tobytes(), got))
    for T, got in out[1:]:
        if T == out[0][0]:
            assert got == out[0][1]


def test_state_errors(api, frames):
    from rsreg_amd import lib as L
    src, tgt = frames
    ctx = api.Context(0)
    score, nr = np.zeros(1), np.zeros(1, np.uint64)
    sums = np.zeros(2)
    lib = L.lib()
    assert lib.rsreg_icp_fitness_score(ctx.h, DBL_MAX, score.ctypes.data_as(L.C.POINTER(L.C.c_double)), None) == L.RSREG_ERR_STATE
    assert lib.rsreg_ndt_fitness_score(ctx.h, DBL_MAX, score.ctypes.data_as(L.C.POINTER(L.C.c_double)), None) == L.RSREG_ERR_STATE
    icp = _align(api, ctx, src, tgt, gate=0.05)
    assert lib.rsreg_icp_fitness_sums(ctx.h, DBL_MAX, sums.ctypes.data_as(L.C.POINTER(L.C.c_double))) == 0
    assert sums[0] == icp.fitnessScore()[1]
    keep, p, n, s = api._records(src)
    assert lib.rsreg_icp_set_source(ctx.h, p, n, s, 0) == 0   # a new source, not aligned yet
    assert lib.rsreg_icp_fitness_sums(ctx.h, DBL_MAX, sums.ctypes.data_as(L.C.POINTER(L.C.c_double))) == L.RSREG_ERR_STATE
    icp2 = api.IterativeClosestPoint(ctx)
    with pytest.raises(L.RsregError):
        icp2.getFitnessScore()
    icp.setInputSource(src)
    with pytest.raises(L.RsregError):
        icp.getFitnessScore()


def test_no_side_effects_on_the_next_alignment(api, frames):
    """An alignment after a fitness call (same target, no new set_target) gives the same 4x4 bits and the same number of search
    launches as one after no such call."""
    src, tgt = frames
    runs = []
    for call in (False, True):
        ctx = api.Context(0)
        icp = _align(api, ctx, src, tgt, gate=0.05)
        if call:
            icp.getFitnessScore()
            icp.getFitnessScore(1e-5)
        icp.setInputSource(src)
        icp.align()
        runs.append((icp.getFinalTransformation().tobytes(), icp.result.n_nn_launches, icp.result.iterations))
    assert runs[0] == runs[1]


def _ndt(api, ctx, src, tgt, resolution=1.0, reference=True):
    n = api.NormalDistributionsTransform(ctx)
    n.params = api.ndt_params(reference=reference)
    n.setResolution(resolution)
    n.setInputSource(src if not isinstance(src, np.ndarray) else _cloud(src))
    n.setInputTarget(tgt if not isinstance(tgt, np.ndarray) else _cloud(tgt))
    n.align()
    return n


def test_ndt_golden_and_synthetic(api, golden, frames):
    g = golden("ndt_small")
    gs, gt = np.ascontiguousarray(g["src"][:, :3], np.float32), np.ascontiguousarray(g["tgt"][:, :3], np.float32)
    ctx = api.Context(0)
    n = _ndt(api, ctx, gs, gt)
    T = n.getFinalTransformation()
    for r in (DBL_MAX, 0.01):
        _check_close(n.fitnessScore(r), _expected(api, ctx, gs, gt, T, r))
    # a synthetic pair, with an ICP alignment of the same context before and after the NDT fitness call
    src, tgt = frames
    ctx = api.Context(0)
    icp = _align(api, ctx, src, tgt, gate=0.05)
    T_icp, s_icp = icp.getFinalTransformation().tobytes(), icp.fitnessScore()
    n = _ndt(api, ctx, src, tgt)
    _check_close(n.fitnessScore(), _expected(api, ctx, _xyz(src), _xyz(tgt), n.getFinalTransformation()))
    icp.setInputSource(src)
    icp.setInputTarget(tgt)
    icp.align()
    assert icp.getFinalTransformation().tobytes() == T_icp
    assert icp.fitnessScore() == s_icp
    with pytest.raises(Exception):
        api.NormalDistributionsTransform(ctx).getFitnessScore()


def test_two_ranks_block_sums_add_up(api):
    """Two contexts holding the two blocks of the source: their block sums (rsreg_icp_fitness_sums, never all-reduced) add up to
    the one-GPU sums, and sharded_fitness_score over them is the one-GPU score (exact on the lattice)."""
    from rsreg_amd import sharded
    src, tgt = far_lattice(70_001)
    one = _align(api, api.Context(0), src, tgt)
    want_sums = one.fitness_sums()
    ranks = []
    for r in range(2):
        lo, hi = sharded.shard_range(len(src), r, 2)
        ranks.append(_align(api, api.Context(0), src[lo:hi], tgt))
    b0, b1 = ranks[0].fitness_sums(), ranks[1].fitness_sums()
    np.testing.assert_array_equal(b0 + b1, want_sums)
    assert sharded.sharded_fitness_score(ranks[0], lambda a: a + b1) == one.fitnessScore()


def test_cpp_adaptor_get_fitness_score(api, tmp_path):
    """include/rsreg/pcl_compat.hpp: getFitnessScore() on IterativeClosestPoint (host and device clouds) and on
    NormalDistributionsTransform, through a small g++ program."""
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "fitness_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "fitness_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    src, tgt = far_lattice(50_000)
    src = np.where(np.isfinite(src), src, np.float32(0.5)).astype(np.float32)   # (the program writes finite records only)
    src.tofile(str(tmp_path / "src.bin"))
    tgt.tofile(str(tmp_path / "tgt.bin"))
    r = subprocess.run([exe, str(tmp_path / "src.bin"), str(tmp_path / "tgt.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    vals = dict(l.split() for l in r.stdout.strip().splitlines())
    want = F.fitness(src, tgt)
    assert float.fromhex(vals["icp_host"]) == want[0]
    assert float.fromhex(vals["icp_host_range"]) == F.fitness(src, tgt, 0.9)[0]
    assert float.fromhex(vals["icp_device"]) == want[0]
    assert vals["state_error"] == "1"
    ctx = api.Context(0)
    n = _ndt(api, ctx, src, tgt, reference=False)   # (the program's NDT runs on the default parameters)
    assert float.fromhex(vals["ndt"]) == n.getFitnessScore()
