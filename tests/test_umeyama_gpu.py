"""The device forms of the Umeyama solve on the table of tests/umeyama_cases.py (flat, thin, mirrored, far, half-turned,
collinear and coincident matches): umeyama_from_sums on one lane (what k_icp_solve runs) and umeyama_wave on a full wave
(what k_final_reduce_solve runs), through tests/cpp/solve.hip -- icp_kernels.hpp compiled as it is, one launch, a wave per
case -- bit for bit against the host form (tests/cpp/linalg_runner.cpp) from the same V, and against the 60-digit reference
(tests/umeyama_ref.py) with the bound tests/test_umeyama_cpu.py derives.  Then through the product: rsreg_icp_update with the
table's sums in sequence inside a live context, and whole alignments of clouds whose nearest-neighbour map is the identity
by construction: pipelines 0, 1 and 2, pipeline 2 behind a single-rank communicator (the k_icp_solve path), and
rsreg_icp_align_records and rsreg_icp_align called by hand.

Every GPU step runs once; nothing is retried."""
import numpy as np
import pytest

import umeyama_cases as uc
import umeyama_ref as ur
from umeyama_cases import check_rigid, expected

IDS = [c["id"] for c in uc.CASES]
PINNED = [c["id"] for c in uc.CASES if c["posed"] == "well" or c["identity"]]
ILL = [c["id"] for c in uc.CASES if c["posed"] == "ill"]
STARTS = ("from-identity", "from-far", "after-full")


@pytest.fixture(scope="module")
def api(rs):
    from rsreg_amd import api as a, lib
    lib.build()
    if a.device_count() < 1:
        pytest.fail("no HIP device: the product has no CPU fallback")
    return a


@pytest.fixture(scope="module")
def refs():
    return {c["id"]: ur.from_pairs(c["P"], c["Q"]) for c in uc.CASES}


def test_harness_compiles_for_gfx950(rs):
    """CPU: tests/cpp/solve.hip still compiles against icp_kernels.hpp as it is."""
    blob = open(uc.build_solve(), "rb").read()
    assert b"gfx950" in blob and b"solve_cases" in blob


@pytest.fixture(scope="module")
def both(api):
    """Every case from three starts -- V = I, an orthogonal V far from I, the V a `full` solve left -- on the host
    (linalg_runner) and in both device forms (solve.hip, one launch)."""
    uc.build_runner()
    so = uc.build_solve()
    S = np.array([c["sums"] for c in uc.CASES])
    n = len(S)
    v_far = uc.orthonormalised(uc.V_ARBITRARY)
    (after,) = uc.run_runner([(2, v_far, uc.BY_ID["full-n1000"]["sums"][None])])
    starts = {"from-identity": uc.IDENT, "from-far": v_far, "after-full": after["V"][0].copy()}
    host = uc.run_runner([(2, starts[k], s[None]) for k in STARTS for s in S])
    dev = uc.run_solve(np.tile(S, (3, 1)), np.concatenate([np.tile(starts[k], (n, 1)) for k in STARTS]), so)
    out = {}
    for a, k in enumerate(STARTS):
        for i, c in enumerate(uc.CASES):
            h = host[a * n + i]
            j = a * n + i
            out[(k, c["id"])] = {"host_T": h["T"][0], "host_V": h["V"][0], "host_ok": int(h["ok"][0, 0]),
                                 "lane_T": dev["T_lane"][j], "lane_V": dev["V_lane"][j], "lane_ok": int(dev["ok_lane"][j]),
                                 "wave_T": dev["T_wave"][j], "wave_V": dev["V_wave"][j], "wave_ok": int(dev["ok_wave"][j])}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("cid", IDS)
def test_device_forms_are_the_host_form_bit_for_bit(both, cid, start):
    """Host and device share the source: the same 16 floats and the same 9 doubles of V, from the same V."""
    r = both[(start, cid)]
    assert r["host_ok"] == r["lane_ok"] == r["wave_ok"] == 1
    np.testing.assert_array_equal(r["lane_T"], r["host_T"])
    np.testing.assert_array_equal(r["lane_V"], r["host_V"])
    np.testing.assert_array_equal(r["wave_T"], r["host_T"])
    np.testing.assert_array_equal(r["wave_V"], r["host_V"])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("lane", "wave"))
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("cid", PINNED)
def test_device_forms_match_reference(both, refs, cid, start, form):
    T = uc.T_rowmajor(both[(start, cid)][form + "_T"])
    Tref, B = expected(uc.BY_ID[cid], refs[cid])
    err = np.abs(T.astype(np.float64) - Tref)
    assert (err <= B).all(), "worst error / bound %.3g\n%s" % ((err[:3] / B[:3]).max(), T)
    check_rigid(T)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ILL)
def test_device_forms_on_ill_posed_cases_are_rigid(both, cid):
    """Rigidity only: centroid onto centroid and the residual of the ill-posed rows are asserted on the host forms
    (tests/test_umeyama_cpu.py), and the device forms are those bit for bit (above)."""
    for start in STARTS:
        for form in ("lane", "wave"):
            check_rigid(uc.T_rowmajor(both[(start, cid)][form + "_T"]))


# ------------------------------------------------------------------------------------------------ through the product
def cloud(rs, xyz):
    pts = np.zeros(len(xyz), rs.POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = np.asarray(xyz, np.float32).T
    pts["w"] = 1.0
    return rs.PointCloud(pts, width=len(pts), height=1, is_dense=True)


def grid_points(nx, ny, step=0.25):
    return np.array([[i * step, j * step, 0.0] for i in range(nx) for j in range(ny)])


def scenes():
    """(name, source, target, posed): target points at least 0.2 m apart (but `one-point`: one target point), the source the
    target moved by less than 2 cm everywhere; gate 0.1 m: the nearest-neighbour map is the identity by construction."""
    tilt = uc.rot([1.0, -2.0, 0.5], 25.0)
    g = np.random.default_rng(11)
    flat = grid_points(16, 16)
    out = []

    def add(name, body, origin, posed="well", far=False, identity=False, deg=0.2):
        Q = (body + origin).astype(np.float32)
        c = Q.astype(np.float64).mean(axis=0)
        R = uc.rot([0.3, -0.4, 1.0], deg)
        P = uc.move(Q, R, c - R @ c + [0.004, -0.003, 0.002])
        assert np.abs(P.astype(np.float64) - Q).max() < 0.02
        out.append({"name": name, "P": P, "Q": Q, "posed": posed, "far": far, "identity": identity})
    add("wall", flat @ tilt.T, [0.1, 0.4, 2.0])
    for scale in (1e-3, 1e-6):
        slab = flat + np.c_[np.zeros((256, 2)), g.uniform(-1, 1, 256) * scale]
        add("thin-%g" % scale, slab @ tilt.T, [0.1, 0.4, 2.0])
    add("far", flat @ tilt.T, [40.0, -30.0, 60.0], far=True)
    add("line", np.arange(128)[:, None] * np.array([0.25, 0.125, 0.0625]), [0.5, -0.25, 1.0], posed="ill", deg=0.03)
    tri = np.array([[0.0, 0.0, 1.0], [0.5, 0.0, 1.25], [0.0, 0.75, 1.0]])
    add("triangle", tri, [0.0, 0.0, 0.0])
    out.append({"name": "one-point", "P": np.tile(np.array([0.5, -0.25, 2.0], np.float32), (128, 1)),
                "Q": np.array([[0.53125, -0.25, 1.96875]], np.float32), "posed": "well", "far": False, "identity": True})
    return out


SCENES = {s["name"]: s for s in scenes()}


@pytest.fixture(scope="module")
def comm_ctx(api):
    """A context with a single-rank communicator: the device loop then runs reduce, all-reduce and k_icp_solve (the one-lane
    form, its state kept in IcpDevState) instead of k_final_reduce_solve (icp.hip launch_fused: device_loop && ctx->comm)."""
    ctx = api.Context(0)
    ctx.comm_init(api.comm_unique_id(), 0, 1)
    return ctx


# the ways through the product: (pipeline_mode, communicator?, entry point called by hand or None for ICP.align())
WAYS = {"staged": (0, False, None), "fused": (1, False, None), "device-loop": (2, False, None), "device-loop-comm": (2, True, None),
        "rsreg_icp_align_records": (0, False, "rsreg_icp_align_records"), "rsreg_icp_align": (0, False, "rsreg_icp_align")}


def align(api, rs, sc, way, iters, comm_ctx):
    """(final transform, the sums of the last iteration, iterations) of one alignment, identity guess, fixed count."""
    import ctypes as C
    from rsreg_amd import lib as _l
    pipeline, with_comm, entry = WAYS[way]
    icp = api.IterativeClosestPoint(comm_ctx) if with_comm else api.IterativeClosestPoint()
    icp.params = api.icp_params(max_iterations=iters, criteria_mode=1, pipeline_mode=pipeline, max_correspondence_distance=0.1)
    src = cloud(rs, sc["P"])
    icp.setInputSource(src)
    icp.setInputTarget(cloud(rs, sc["Q"]))
    if entry is None:
        icp.align()
        res = icp.result
    else:
        icp._sync_inputs()
        res = _l.IcpResult()
        recs = np.ascontiguousarray(src.points)
        if entry == "rsreg_icp_align_records":
            out = np.empty(len(recs), recs.dtype)
            rc = _l.lib().rsreg_icp_align_records(icp.ctx.h, None, C.byref(icp.params), C.byref(res), recs.ctypes.data, out.ctypes.data,
                                                  out.dtype.itemsize)
        else:
            out = recs.copy()
            rc = _l.lib().rsreg_icp_align(icp.ctx.h, None, C.byref(icp.params), C.byref(res), out.ctypes.data, out.dtype.itemsize)
        _l.check(rc, icp.ctx.h)
        assert np.isfinite(out["x"]).all() and np.isfinite(out["y"]).all() and np.isfinite(out["z"]).all()
    return np.asarray(api._rowmajor(res.transform), np.float32), np.array(res.sums_last), int(res.iterations)


def mul32(a, b):
    """host_linalg.hpp mul(): c = a b in float32, ((a0 b0 + a1 b1) + a2 b2) + a3 b3, no FMA."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    c = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            s = np.float32(a[i, 0] * b[0, j])
            for k in (1, 2, 3):
                s = np.float32(s + np.float32(a[i, k] * b[k, j]))
            c[i, j] = s
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_alignment_of_matched_clouds(api, rs, comm_ctx, name):
    sc = SCENES[name]
    n = len(sc["P"])
    # the premise first: every source record's nearest target point is its own
    icp = api.IterativeClosestPoint()
    icp.params = api.icp_params(max_iterations=1, criteria_mode=1, pipeline_mode=0, max_correspondence_distance=0.1)
    icp.setInputSource(cloud(rs, sc["P"]))
    icp.setInputTarget(cloud(rs, sc["Q"]))
    icp.begin()
    idx, _ = icp.search()
    own = np.arange(n) if len(sc["Q"]) == n else np.zeros(n, int)
    np.testing.assert_array_equal(idx, own)
    icp.sums()
    icp.end()
    Qm = sc["Q"][own]

    # one iteration, identity guess: the solve alone
    ref = ur.from_pairs(sc["P"], Qm)
    one = {w: align(api, rs, sc, w, 1, comm_ctx) for w in WAYS}
    for w in WAYS:
        np.testing.assert_array_equal(one[w][0], one["staged"][0], err_msg=w)
        np.testing.assert_array_equal(one[w][1], one["staged"][1], err_msg=w)
        assert one[w][2] == 1, w
    T1, sums1, it1 = one["device-loop"]
    assert it1 == 1 and sums1[0] == n
    check_rigid(T1)
    case = {"identity": sc["identity"], "far": sc["far"]}
    if sc["posed"] == "well":
        Tref, B = expected(case, ref)
        err = np.abs(T1.astype(np.float64) - Tref)
        assert (err <= B).all(), "worst error / bound %.3g\n%s" % ((err[:3] / B[:3]).max(), T1)
    else:
        R, t = T1[:3, :3].astype(np.float64), T1[:3, 3].astype(np.float64)
        pmax = float(np.abs(sc["P"]).max())
        slack = 3 * pmax * 2.0 ** -24 + 0.5 * ur.ulp32(t).max() + ur.C * ur.EPS * (1 + 3 * pmax)
        assert ur.rms_residual(sc["P"], Qm, R, t) <= ur.rms_residual(sc["P"], Qm, ref["R"], ref["t"]) + np.sqrt(3) * slack

    # two and three iterations: every way through the product bit for bit, and each step the increment of its own sums on the last
    prev = T1
    for k in (2, 3):
        runs = {w: align(api, rs, sc, w, k, comm_ctx) for w in WAYS}
        for w in WAYS:
            np.testing.assert_array_equal(runs[w][0], runs["staged"][0], err_msg="%s, %d iterations" % (w, k))
            np.testing.assert_array_equal(runs[w][1], runs["staged"][1], err_msg="%s, %d iterations" % (w, k))
            assert runs[w][2] == k, w
        Tk, sums_k, it_k = runs["device-loop"]
        assert it_k == k and sums_k[0] == n
        check_rigid(Tk)
        if sc["posed"] == "well" and not sc["identity"]:
            inc = ur.from_sums(sums_k)
            Tinc = ur.T_of(inc).astype(np.float32)
            want = mul32(Tinc, prev).astype(np.float64)
            # the increment within its bound, carried through the product; the float product rounds 4 products and 3 sums
            # on either side
            B = ur.bound(inc, sc["far"]) @ np.abs(prev.astype(np.float64)) + 8 * 2.0 ** -24 * (np.abs(Tinc.astype(np.float64)) @ np.abs(prev.astype(np.float64)))
            err = np.abs(Tk.astype(np.float64) - want)
            assert (err[:3] <= B[:3]).all(), "iteration %d: worst error / bound %.3g" % (k, (err[:3] / B[:3]).max())
        if sc["identity"]:
            np.testing.assert_array_equal(Tk[:3, :3], np.eye(3, dtype=np.float32))
        prev = Tk


@pytest.mark.gpu
def test_update_in_a_live_context_is_the_host_warm_form(api, rs):
    """rsreg_icp_update with the table's sums in sequence (V carried from each to the next inside the context) against the
    same sequence through linalg_runner."""
    uc.build_runner()
    sc = SCENES["wall"]
    icp = api.IterativeClosestPoint()
    icp.params = api.icp_params(max_iterations=100000, criteria_mode=1, pipeline_mode=0, max_correspondence_distance=0.1)
    icp.setInputSource(cloud(rs, sc["P"]))
    icp.setInputTarget(cloud(rs, sc["Q"]))
    icp.begin()
    S = np.array([c["sums"] for c in uc.CASES] + [s for _, _, s in uc.slow_sequence()])
    (want,) = uc.run_runner([(2, uc.IDENT, S)])
    for k, s in enumerate(S):
        t_inc, done = icp.update(s)
        assert not done
        np.testing.assert_array_equal(np.asarray(t_inc, np.float32), uc.T_rowmajor(want["T"][k]), err_msg="step %d" % k)
    icp.end()
