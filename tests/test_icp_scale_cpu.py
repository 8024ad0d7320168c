"""The ICP correspondence search across the float32 range, on the CPU: everything tests/test_icp_scale_gpu.py relies on, asserted on
the references alone.

  * tests/icp_grid_layout.py (the Python restatement of csrc/icp_grid_plan.hpp) equals tests/cpp/icp_grid_plan.cpp, which runs the
    header itself (g++, no HIP), on every case, under every set of switches, for the first and the refined pass, and on random boxes.
  * tests/icp_search_ref.py equals the brute force of tests/test_nn_fuzz_gpu.py.
  * Family A is exactly covariant: the indices of scale 1, d2 times 2^2e, the 17 sums times their powers of two.
  * Every family has cases that accept pairs, cases that reject pairs and cases with ties.
  * The cost cap: OVER_CAP is what the cost model says, and every case that goes to a GPU is under it for every index kind.
  * The GPU table takes both index kinds and all three far searches (per the plan), and accepted pairs beyond ring 1 exist on each.
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import icp_grid_layout as L
import icp_scale_cases as K
import icp_search_ref as R
import scale_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsense-pointcloud_amd", "csrc")
IDS = [c.id for c in K.CASES]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("icp_grid_plan") / "icp_grid_plan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "icp_grid_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


def _hex(v):
    v = float(v)
    return "inf" if v == math.inf else "-inf" if v == -math.inf else v.hex()


def _run(program, rows):
    """rows: (mn, mx, nfin, max_dist, refine, tun, n_unique, n_cells) -> [(Plan fields ..., refine factor)] from the header itself."""
    out = []
    for s in range(0, len(rows), 100):
        args = []
        for mn, mx, nfin, max_dist, refine, tun, n_unique, n_cells in rows[s:s + 100]:
            args += [_hex(v) for v in np.asarray(mn, np.float32)] + [_hex(v) for v in np.asarray(mx, np.float32)]
            args += [str(int(nfin)), _hex(max_dist), _hex(refine), _hex(tun.cell_cap), "1" if tun.wide_cells else "0", str(int(tun.dense_max_cells)),
                     str(int(n_unique)), str(int(n_cells))]
        r = subprocess.run([program] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-3000:]
        for line in r.stdout.strip().splitlines():
            w = line.split()
            f = [float.fromhex(x) for x in w[:5]]
            out.append((f[0], f[1], tuple(f[2:5]), tuple(int(x) for x in w[5:8]), int(w[8]), int(w[9]), bool(int(w[10])), bool(int(w[11])), float.fromhex(w[12])))
    assert len(out) == len(rows)
    return out


def _same(program, rows):
    got = _run(program, rows)
    for row, g in zip(rows, got):
        mn, mx, nfin, max_dist, refine, tun, n_unique, n_cells = row
        p = L.plan(mn, mx, nfin, max_dist, refine, tun)
        mine = (float(p.cell), float(p.inv_cell), tuple(float(v) for v in p.origin), tuple(p.dims), p.max_ring, p.index_kind, p.bounded, p.served,
                L.refine_factor(n_unique, n_cells))
        assert mine == g, (row, mine, g)


def test_restatement_equals_the_header_on_every_case(program):
    rows = []
    for c in K.CASES:
        mn, mx, nfin = L.box_of(K.target(c.id))
        for tun in K.TUNABLE_SETS.values():
            first = L.plan(mn, mx, nfin, K.gate(c.id), 1.0, tun)
            n_unique, n_cells = L.occupancy(K.target(c.id), first)
            for refine in (1.0, L.refine_factor(n_unique, n_cells), 0.2, 0.61):
                rows.append((mn, mx, nfin, K.gate(c.id), refine, tun, n_unique, n_cells))
    _same(program, rows)


def test_restatement_equals_the_header_on_random_boxes(program):
    rng = np.random.default_rng(4400)
    rows = []
    for i in range(600):
        scale = 2.0 ** rng.integers(-60, 60)
        mn = (rng.standard_normal(3) * scale).astype(np.float32)
        mx = (mn.astype(np.float64) + np.abs(rng.standard_normal(3)) * scale * 2.0 ** rng.integers(-8, 8, 3)).astype(np.float32)
        gate = [R.UNBOUNDED, math.inf, 0.0, float(scale * 2.0 ** rng.integers(-12, 4)), 0.05][i % 5]
        tun = L.Tunables([0.014, 0.003, 0.1][i % 3], bool(i % 7), [1 << 28, 0, 2000000][i % 3], True)
        rows.append((mn, np.maximum(mn, mx), int(rng.integers(1, 3000000)), gate, [1.0, 0.2, 0.5][i % 3], tun, int(rng.integers(0, 5000)), int(rng.integers(0, 300))))
    _same(program, rows)


def test_restated_constants_are_the_headers():
    def text(f):
        return open(os.path.join(CSRC, f)).read()
    plan_h = text("icp_grid_plan.hpp")
    assert float(re.search(r"kIcpPlanMargin = ([0-9.]+)f", plan_h).group(1)) == pytest.approx(float(L.CELL_MARGIN), abs=1e-9)
    assert float(re.search(r"kCellMargin = ([0-9.]+)f", text("records.hpp")).group(1)) == pytest.approx(float(L.CELL_MARGIN), abs=1e-9)
    assert float(re.search(r"kIcpCoordMax = ([0-9.]+)f", plan_h).group(1)) == float(L.COORD_MAX)
    assert float(re.search(r"kIcpAxisCells = ([0-9.]+);", plan_h).group(1)) == L.AXIS_CELLS
    assert float.fromhex(re.search(r"kIcpCellMax = (0x1p[0-9]+)f;", plan_h).group(1)) == float(L.CELL_MAX)
    t = text("tunables.hpp")
    assert float(re.search(r"double cell_cap = ([0-9.]+);", t).group(1)) == L.DEFAULT.cell_cap
    assert re.search(r"long long dense_max_cells = 1ll << 28;", t) and L.DEFAULT.dense_max_cells == 1 << 28


def test_reference_is_the_brute_force_of_the_fuzz_test():
    import test_nn_fuzz_gpu as F
    for cid in ("A-holes*2^20-bounded", "A-copies*2^-20-unbounded", "B-2^23-xyz-bounded", "C-two_at_3e38-bounded", "D-far-unbounded"):
        ref = K.ref(cid)
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            idx, d2 = F.brute(K.source(cid)[:300], K.target(cid), K.gate(cid))
        np.testing.assert_array_equal(ref.idx[:300], idx)
        np.testing.assert_array_equal(ref.d2[:300], d2)


# ------------------------------------------------------------------------------------------------ family A: covariance
@pytest.mark.parametrize("gate_kind", ("bounded", "unbounded"))
@pytest.mark.parametrize("name", S.BASES)
def test_family_a_is_exactly_covariant(name, gate_kind):
    src = K.base_source(name).astype(np.float32)
    assert np.isfinite(src).all()            # (holes: built from finite rows)
    gate1 = 0.03 * K._extent(S.base(name)) if gate_kind == "bounded" else R.UNBOUNDED
    one = R.search(src, S.base(name), gate1)
    power = np.array([0] + [1] * 6 + [2] * 10)
    for e in S.WINDOW:
        ref = K.ref("A-%s*2^%d-%s" % (name, e, gate_kind))
        np.testing.assert_array_equal(ref.idx, one.idx)
        np.testing.assert_array_equal(ref.d2, np.ldexp(one.d2, 2 * e))
        np.testing.assert_array_equal(ref.near_d2, np.ldexp(one.near_d2, 2 * e))
        np.testing.assert_array_equal(ref.sums, np.ldexp(one.sums, power * e))
        np.testing.assert_array_equal(ref.sums_abs, np.ldexp(one.sums_abs, power * e))


# ------------------------------------------------------------------------------------------------ what the cases hold
@pytest.mark.parametrize("family", "ABCD")
def test_family_accepts_rejects_and_ties(family):
    ids = [c.id for c in K.CASES if c.family == family]
    accepted = [i for i in ids if (K.ref(i).idx >= 0).any()]
    rejected = [i for i in ids if ((K.ref(i).idx < 0) & (K.ref(i).near_idx >= 0)).any()]
    tied = [i for i in ids if K.ties(i) > 0]
    assert accepted and rejected and tied, (len(accepted), len(rejected), len(tied))


def test_sizes_and_special_records():
    for c in K.CASES:
        assert len(K.target(c.id)) <= 2000 and len(K.source(c.id)) <= 1500
    assert not R.finite_rows(K.target("A-holes*2^20-bounded")).all()
    ref = K.ref("D-far-bounded")
    assert (ref.idx == -1).all() and (ref.near_idx >= 0).all()
    far = K.ref("D-far-unbounded")
    assert (far.idx >= 0).any() and np.isinf(far.near_d2).any()       # (beyond 2^64 m d2 overflows: +inf is rejected by sqrt(DBL_MAX))
    assert np.isinf(K.ref("C-uniform*2^66-bounded").near_d2).any() or np.isinf(K.ref("C-uniform*2^70-bounded").near_d2).any()
    assert (K.ref("C-uniform*2^-120-unbounded").d2 == 0).all()


# ------------------------------------------------------------------------------------------------ the cost cap
def test_over_cap_is_what_the_model_says():
    assert sorted(i for i in IDS if not K.under_cap(i)) == sorted(K.OVER_CAP)
    assert all(BY.gate_kind == "unbounded" for BY in (K.BY_ID[i] for i in K.OVER_CAP))
    assert any(K.BY_ID[i].family == "A" and K.BY_ID[i].e >= 20 for i in K.OVER_CAP)
    assert any(K.BY_ID[i].name in S.MIXED for i in K.OVER_CAP)


def test_every_gpu_case_is_under_the_cap_for_every_index_kind():
    ids = K.gpu_ids()
    assert ids and not set(ids) & set(K.OVER_CAP)
    for cid in ids:
        n_points = int(R.finite_rows(K.target(cid)).sum())
        kinds = set()
        for t in K.TUNABLE_SETS:
            p = K.plan(cid, t)
            kinds.add(p.index_kind)
            q = L.cost_bound(p, K.limit_of(cid), n_points)
            assert q <= K.PER_QUERY_CAP and q * len(K.source(cid)) * K.SEARCHES <= K.PER_CASE_CAP, (cid, t, q)
        assert kinds == {0, 1}, (cid, kinds)         # (both index kinds are modelled for every case)


def test_cost_model_grows_as_the_loops_do():
    p = K.plan("A-uniform*2^20-unbounded")
    assert p.index_kind == 0 and L.far_search(p) == "hash_shells"
    nb = [(d + 3) >> 2 for d in p.dims]
    whole = L.far_bound(p, math.inf)
    assert whole >= nb[0] * nb[1] * nb[2]                       # an unbounded search can probe every brick of the grid
    assert L.far_bound(p, 0.5 * float(p.cell)) == 0                # inside ring 1: no far search
    near = L.far_bound(p, 100.0 * float(p.cell))                 # 100 cells: 27 shells of bricks
    assert (2 * 26 + 1) ** 3 <= near <= 4 * (2 * 27 + 1) ** 3
    d = K.plan("B-2^10-x-unbounded")
    assert L.far_search(d) == "dense_rows" and L.far_bound(d, math.inf) == (2 * d.max_ring + 1) ** 2
    assert L.far_bound(K.plan("B-2^10-x-bounded"), 0.05) == 108


# ------------------------------------------------------------------------------------------------ which searches the GPU table takes
def _beyond_ring1(cid, p):
    """Accepted pairs of the reference farther than a cell from their query: matches only a search beyond ring 1 can find."""
    ref = K.ref(cid)
    return int(((ref.idx >= 0) & (np.sqrt(ref.d2.astype(np.float64)) > float(p.cell))).sum())


def test_gpu_table_takes_both_index_kinds_and_all_three_far_searches():
    taken = {}
    for cid in K.gpu_ids():
        for t in ("default", "force_hash"):
            p = K.plan(cid, t)
            taken.setdefault((t, L.far_search(p)), []).append((cid, _beyond_ring1(cid, p)))
    assert {k for t, k in taken if t == "default"} >= {"dense_rows", "dense_blocks"}
    assert {k for t, k in taken if t == "force_hash"} >= {"hash_shells"}      # (tests/test_index_paths_gpu.py: RSREG_FORCE_HASH=1)
    for key in (("default", "dense_rows"), ("default", "dense_blocks"), ("force_hash", "hash_shells")):
        assert any(n > 0 for _, n in taken[key]), key
    assert all(K.plan(cid, "default").index_kind == 1 and K.plan(cid, "force_hash").index_kind == 0 for cid in K.gpu_ids())


def test_served_range_is_the_same_under_every_switch_and_as_stated():
    for c in K.CASES:
        flags = {K.plan(c.id, t).served for t in K.TUNABLE_SETS}
        assert len(flags) == 1, c.id
    refused = set(K.refused_ids())
    # what the header states: a cell above 2^60 m (cell * cell leaves the normal floats), or a box wider than a float
    assert {"C-uniform*2^100-bounded", "C-uniform*2^100-unbounded", "C-one_at_1e30-bounded", "C-two_at_3e38-bounded", "C-wide_and_1e23-bounded"} <= refused
    for cid in refused:
        p = K.plan(cid)
        with np.errstate(over="ignore"):
            wide = not np.isfinite((K.target(cid).max(axis=0) - K.target(cid).min(axis=0)).astype(np.float32)).all()
        assert float(p.cell) > 2.0 ** 60 or wide, cid
    for cid in K.gpu_ids():
        p = K.plan(cid)
        assert 1e-6 <= float(p.cell) <= 2.0 ** 60 and max(p.dims) <= 60004, cid
    assert not set(K.gpu_ids()) & refused and {K.BY_ID[i].family for i in K.gpu_ids()} == set("ABCD")


def test_a_gate_of_plus_infinity_accepts_infinite_distances():
    for cid in K.INF_GATE:
        ref = K.ref(cid)
        inf = np.isinf(ref.near_d2)
        assert inf.any() and (ref.idx[inf] == 0).all() and np.isinf(ref.d2[inf]).all()      # +inf ties with +inf: record 0, accepted
        assert (K.ref("D-far-unbounded").idx[inf] == -1).all()                             # (sqrt(DBL_MAX) rejects the same pairs)
        assert K.served(cid) and K.under_cap(cid) and cid not in K.gpu_ids()


def test_far_queries_lie_on_both_sides_of_the_far_boundary():
    """kFarCells of csrc/icp_kernels.hpp: family D has queries inside it (the bounds serve them) and outside (every point is scored)."""
    far_cells = float(re.search(r"kFarCells = ([0-9.]+)f;", open(os.path.join(CSRC, "icp_kernels.hpp")).read()).group(1))
    for t in K.TUNABLE_SETS:
        p = K.plan("D-far-unbounded", t)
        u = np.stack([L.cell_pos(K.source("D-far-unbounded")[:, k], p.origin[k], p.inv_cell) for k in range(3)], axis=1)
        out = np.maximum(-u, u - np.asarray(p.dims, np.float32)).max(axis=1)
        assert (out < far_cells).any() and (out > far_cells).any() and (out > 1e30).any(), t


def test_update_check_has_well_posed_cases_in_families_a_and_b():
    """tests/test_icp_scale_gpu.py checks update() where the reference solve is well posed: from the reference's sums, that is every
    case of families A and B it runs."""
    import umeyama_ref as U
    power = np.array([0] + [1] * 6 + [2] * 10)
    for cid in K.gpu_ids():
        c = K.BY_ID[cid]
        if c.family in "AB":
            sums = np.ldexp(K.ref(cid).sums, -power * (c.e if c.family == "A" else 0))
            assert sums[0] >= 3 and np.isfinite(U.kappa(U.from_sums(sums))), cid


def test_a_gate_beyond_int_range_over_the_cap_still_gets_eight_parts():
    """(int)ceil(gate / cap) above 2^31 was undefined and came out as one part: A-*2^40-bounded had 34 x 26 x 13 cells where 2^20 has
    258 x 194 x 91.  icp_grid_plan clamps as a double: the same eight parts at every scale of the window from 2^20 up."""
    for e in (20, 40, 55):
        p = K.plan("A-uniform*2^%d-bounded" % e)
        assert p.dims == (258, 194, 91) and p.max_ring == 8 and p.cell == np.float32(K.gate("A-uniform*2^%d-bounded" % e) * 1.04 / 8)
