"""GeneralizedIterativeClosestPoint6D on the GPU (rsreg_cloud_lab: k_cloud_lab; rsreg_gicp6d_*: k_nn_search6 over the 6-D index,
k_source_unmerge) against tests/gicp6d_ref.py, the numpy restatement of include/rsreg.h's GICP6D section.

Colour: the kernel's bytes are rsreg_rgb_to_lab's (held bit-equal to the reference on all 2^24 colours by tests/test_gicp6d_cpu.py).
Search: indices and d6 of rsreg_gicp_search against the float32 brute force over ALL target records, bit for bit -- the contract is
an exact rule (smallest (d6, index), one rounding per operation), so nothing is tolerated.  Sums [1]: the f64 sum of the kept d6,
within (N + 16) * 2^-53 * sum|term| of the reference's (gicp_ref.sums_bound, as the GICP test).  Whole alignment on the scene
tests/test_gicp6d_cpu.py pins: within 1e-4 Frobenius of the 6-D reference (the CPU test shows the margin), and the 3-D class on
the same clouds more than 5e-3 from the truth.
"""
import numpy as np
import pytest

import filters_ref
import gicp6d_cases as GC6
import gicp6d_ref as R
import gicp_cases as GC
import gicp_ref as G
import plane_cases as PC

pytestmark = pytest.mark.gpu
GATE = 0.05


@pytest.fixture(scope="module")
def api():
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    return api


@pytest.fixture(scope="module")
def ctxs(api):
    return api.Context(0), api.Context(0)


def _unit_cov(n):
    return GC.plane_covariances(np.tile(np.array([0.0, 0.0, 1.0]), (n, 1)))


def make6(api, ctx, src, tgt, lab_s, lab_t, gate, weight, **params):
    g = api.GeneralizedIterativeClosestPoint6D(ctx, lab_weight=weight)
    g.setMaxCorrespondenceDistance(gate)
    for k, v in params.items():
        setattr(g.gparams, k, v)
    g.setInputSource(PC.cloud(src))
    g.setInputTarget(PC.cloud(tgt))
    g.setSourceCovariances(_unit_cov(len(src)))
    g.setTargetCovariances(_unit_cov(len(tgt)))
    g.setSourceLab(lab_s)
    g.setTargetLab(lab_t)
    return g


def search6(api, ctx, src, tgt, lab_s, lab_t, gate, weight, guess=None):
    """(engine idx, d6, reference idx, d6) of one search"""
    g = make6(api, ctx, src, tgt, lab_s, lab_t, gate, weight)
    g.begin(guess)
    idx, d2 = g.search()
    g.end()
    cur = np.ascontiguousarray(src, np.float32).copy()
    if guess is not None:
        fin = np.isfinite(cur).all(axis=1)
        cur[fin] = filters_ref.transform(cur[fin], guess)
    ri, rd = R.nearest6(cur, R.scaled(lab_s, weight), tgt, R.scaled(lab_t, weight), gate)
    return idx, d2, ri, rd


def same(idx, d2, ri, rd):
    bad = np.flatnonzero((idx != ri) | (d2.view(np.uint32) != rd.view(np.uint32)))
    assert not len(bad), (len(bad), bad[:8], idx[bad[:8]], ri[bad[:8]], d2[bad[:8]], rd[bad[:8]])


@pytest.fixture(scope="module")
def boxes():
    src, lab_s = GC6.box_cloud(2000, 21)
    tgt, lab_t = GC6.box_cloud(3000, 22)
    # the source near the target: 1 500 of its records a centimetre or two off, the rest where they fell
    rng = np.random.default_rng(23)
    pick = rng.choice(3000, 1500, replace=False)
    src[:1500] = tgt[pick] + rng.normal(0, 0.012, (1500, 3)).astype(np.float32)
    return src, lab_s, tgt, lab_t


# ---------------------------------------------------------------------------------------------------- colour
class _Raw:
    def __init__(self, points, width, height, is_dense):
        self.points, self.width, self.height, self.is_dense = points, width, height, is_dense


@pytest.mark.parametrize("stride", (20, 32, 48))
def test_cloud_lab_gives_the_host_functions_bytes(api, ctxs, stride):
    rng = np.random.default_rng(stride)
    dt = np.dtype({"names": ["x", "y", "z", "w", "rgba"], "formats": ["<f4"] * 4 + ["<u4"], "offsets": [0, 4, 8, 12, 16], "itemsize": stride})
    for n in (1, 63, 64, 65, 1000):
        pts = np.zeros(n, dt)
        pts["x"], pts["y"], pts["z"] = rng.normal(0, 1, (3, n)).astype(np.float32)
        pts["rgba"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        pts["x"][::7] = np.nan
        pts["z"][3::11] = np.inf
        pts["rgba"][:1] = 0xffffff
        dev = api.DeviceCloud(_Raw(pts, n, 1, False), ctx=ctxs[0])
        out = dev.lab_cloud()
        assert out.info() == (n, 16, n, 1, False)
        rec = np.zeros((n, 4), np.float32)
        from rsreg_amd import lib
        lib.check(lib.lib().rsreg_cloud_download(out.h, rec.ctypes.data, n), ctxs[0].h)
        assert rec[:, :3].tobytes() == api.rgb_to_lab(pts["rgba"]).tobytes() and (rec[:, 3].view(np.uint32) == 0).all()
        assert dev.lab().tobytes() == rec[:, :3].tobytes()
        out.close()
        dev.close()


def test_cloud_lab_refuses_records_without_a_colour(api, ctxs):
    from rsreg_amd import lib
    pts = np.zeros(10, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("w", "<f4")]))
    dev = api.DeviceCloud(_Raw(pts, 10, 1, True), ctx=ctxs[0])
    out = api.DeviceCloud(ctx=ctxs[0])
    assert lib.lib().rsreg_cloud_lab(ctxs[0].h, dev.h, out.h) == lib.RSREG_ERR_INVALID_ARG
    assert lib.lib().rsreg_cloud_lab(ctxs[0].h, dev.h, dev.h) == lib.RSREG_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------------- search
def test_weight_zero_is_the_3d_search(api, ctxs, boxes):
    src, lab_s, tgt, lab_t = boxes
    idx, d2, ri, rd = search6(api, ctxs[0], src, tgt, lab_s, lab_t, GATE, 0.0)
    same(idx, d2, ri, rd)
    p2p = api.IterativeClosestPoint(ctxs[1])
    p2p.setMaxCorrespondenceDistance(GATE)
    p2p.setInputSource(PC.cloud(src))
    p2p.setInputTarget(PC.cloud(tgt))
    p2p.begin()
    i3, d3 = p2p.search()
    p2p.end()
    assert idx.tobytes() == i3.tobytes() and d2.tobytes() == d3.tobytes() and (idx >= 0).sum() > 1000


@pytest.mark.parametrize("weight,gate", ((0.032, GATE), (1.0, GATE), (1.0, 0.5)))
def test_search_is_the_brute_force(api, ctxs, boxes, weight, gate):
    src, lab_s, tgt, lab_t = boxes
    idx, d2, ri, rd = search6(api, ctxs[0], src, tgt, lab_s, lab_t, gate, weight)
    same(idx, d2, ri, rd)
    import plane_ref
    i3, d3 = plane_ref.nearest_brute(src, tgt)
    k = idx >= 0
    differs = int((idx[k] != i3[k]).sum())
    in3 = int((~(d3.astype(np.float64) > gate * gate)).sum())
    print("weight %g, gate %g: %d pairs (%d in 3-D), %d of them not the 3-D nearest" % (weight, gate, int(k.sum()), in3, differs))
    if weight < 1:
        assert k.sum() > 500 and differs > 0
    elif gate == GATE:
        assert k.sum() < 0.1 * in3   # random colours at weight 1 are farther apart than 5 cm: nearly every pair is rejected on d6
    else:
        assert k.sum() > 500 and differs > 0.5 * k.sum()   # colour dominates: the winner is rarely the 3-D nearest


def test_duplicated_target_records(api, ctxs, boxes):
    src, lab_s, tgt, lab_t = boxes
    # every third target record twice more: once with its own colour (the lowest index must win), once with another
    # colour (the colour must decide) -- the copies first, so that the lowest index is not always the original
    t2 = np.concatenate([tgt[::3], tgt, tgt[::3]])
    other = np.roll(lab_t[::3], 1, axis=0)
    l2 = np.concatenate([lab_t[::3], lab_t, other])
    idx, d2, ri, rd = search6(api, ctxs[0], src, t2, lab_s, l2, GATE, 0.032)
    same(idx, d2, ri, rd)
    n3 = len(tgt[::3])
    k = idx >= 0
    assert (idx[k] < n3).any() and (idx[k] >= n3 + len(tgt)).any(), "both kinds of copies win somewhere"
    # a source that sits ON target records with the colour of the differently coloured copy: that copy wins, at d6 = 0
    s2, ls2 = tgt[::3][:200].copy(), other[:200].copy()
    idx, d2, ri, rd = search6(api, ctxs[0], s2, t2, ls2, l2, GATE, 0.5)
    same(idx, d2, ri, rd)
    assert (d2 == 0).all() and (idx >= n3 + len(tgt)).sum() > 150
    # ... and with the original's colour: the first copy (the lowest index)
    idx, d2, ri, rd = search6(api, ctxs[0], s2, t2, lab_t[::3][:200].copy(), l2, GATE, 0.5)
    same(idx, d2, ri, rd)
    assert (d2 == 0).all() and (idx < n3).all()


def test_the_gate_is_applied_to_d6(api, ctxs, boxes):
    _, _, tgt, lab_t = boxes
    rng = np.random.default_rng(31)
    # isolated targets (a coarse lattice, 20 cm apart), sources 3 cm off: inside the 5 cm gate in 3-D ...
    g = np.stack(np.meshgrid(np.arange(8), np.arange(6), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3)
    t = (g * 0.2).astype(np.float32)
    lt = np.zeros((len(t), 3), np.float32)
    s = (t + np.array([0.03, 0.0, 0.0], np.float32)).astype(np.float32)
    ls = np.zeros((len(s), 3), np.float32)
    # ... and a colour difference that lands d6 just outside (0.0401 m in colour for every other source), or just inside
    ls[::2, 0] = 0.0401
    ls[1::2, 0] = 0.0399
    idx, d2, ri, rd = search6(api, ctxs[0], s, t, ls, lt, GATE, 1.0)
    same(idx, d2, ri, rd)
    assert (idx[::2] == -1).all() and (idx[1::2] == np.arange(len(t))[1::2]).all()
    assert (d2[::2] == 0).all() and (d2[1::2].astype(np.float64) <= GATE * GATE).all()


def test_queries_far_outside_the_target(api, ctxs, boxes):
    src, lab_s, tgt, lab_t = boxes
    s = src[:400].copy()
    s[:100] += np.float32(3.0)                    # outside the box, within a wide gate
    s[100:200] *= np.float32(1e4)                 # thousands of cells away
    s[200:220] = np.float32(1e30)                 # where (q - origin) / cell overflows
    s[220:240, 0] = np.nan
    ls = lab_s[:400].copy()
    ls[240:250, 1] = np.nan                       # a source colour that is not finite: no pair
    for gate in (GATE, 5.0):
        idx, d2, ri, rd = search6(api, ctxs[0], s, tgt, ls, lab_t, gate, 0.032)
        same(idx, d2, ri, rd)
        assert (idx[100:250] == -1).all()
    assert (idx[:100] >= 0).any()
    # target colours that are not finite: skipped as candidates
    lt = lab_t.copy()
    lt[::2, 2] = np.nan
    idx, d2, ri, rd = search6(api, ctxs[0], src, tgt, lab_s, lt, 5.0, 0.032)
    same(idx, d2, ri, rd)
    assert (idx[idx >= 0] % 2 == 1).all() and (idx >= 0).all()


def test_one_record_on_either_side(api, ctxs, boxes):
    src, lab_s, tgt, lab_t = boxes
    for gate in (GATE, 5.0):
        same(*search6(api, ctxs[0], src, tgt[:1], lab_s, lab_t[:1], gate, 0.032))
        same(*search6(api, ctxs[0], src[:1], tgt, lab_s[:1], lab_t, gate, 0.032))
    # the one target record under a source record of its colour: matched at d6 = 0 at the narrow gate too
    idx, d2, ri, rd = search6(api, ctxs[0], tgt[:1], tgt[:1], lab_t[:1], lab_t[:1], GATE, 0.032)
    same(idx, d2, ri, rd)
    assert idx.tolist() == [0] and d2[0] == 0


def test_a_second_search_after_an_update(api, ctxs, boxes):
    src, lab_s, tgt, lab_t = boxes
    w = 0.032
    g = make6(api, ctxs[0], src, tgt, lab_s, lab_t, GATE, w)
    guess = G.delta(np.array([0.002, -0.001, 0.003, 0.004, -0.002, 0.001])).astype(np.float32)
    g.begin(guess)
    cs, ct = R.scaled(lab_s, w), R.scaled(lab_t, w)
    idx, d2 = g.search()
    same(idx, d2, *R.nearest6(filters_ref.transform(src, guess), cs, tgt, ct, GATE))
    S = g.gicp_sums(GC.X_TEST)
    assert S[0] == (idx >= 0).sum() and S[0] > 500   # (fewer than 4 pairs would end the alignment where it stands)
    assert not g.update(GC.X_TEST, S, 1)
    T1, _ = G.compose(GC.X_TEST, guess, G.Params())
    idx2, d22 = g.search()
    same(idx2, d22, *R.nearest6(filters_ref.transform(src, T1), cs, tgt, ct, GATE))
    assert (idx2 != idx).any() and (d22 != d2).any()
    res = g.end()
    assert np.array(res.transform, np.float32).reshape(4, 4).T.tobytes() == T1.tobytes()


# ---------------------------------------------------------------------------------------------------- merged sources
def test_a_source_past_the_merge_threshold(api, ctxs, boxes):
    _, _, tgt, lab_t = boxes
    n = 70_001
    rng = np.random.default_rng(41)
    pick = rng.integers(0, len(tgt), n)
    src = (tgt[pick] + rng.normal(0, 0.01, (n, 3))).astype(np.float32)
    src[1::5] = src[::5][:len(src[1::5])]          # exact x, y, z copies of the record in front ...
    lab_s = np.stack([rng.uniform(0, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)], axis=1).astype(np.float32)   # ... with colours of their own
    src[7::1000] = np.nan
    g = make6(api, ctxs[0], src, tgt, lab_s, lab_t, GATE, 0.032)
    g.begin()
    assert g.grid_info().n_source_distinct == n
    idx, d2 = g.search()
    ri, rd = R.nearest6(src, R.scaled(lab_s, 0.032), tgt, R.scaled(lab_t, 0.032), GATE, chunk=2048)
    same(idx, d2, ri, rd)
    a, b = idx[::5][:len(idx[1::5])], idx[1::5]
    assert (a != b).any(), "copies in space with different colours get different pairs somewhere"
    S = g.gicp_sums()
    k = idx >= 0
    terms = d2[k].astype(np.float64)
    assert S[0] == k.sum() and k.sum() > 30_000
    assert abs(S[1] - terms.sum()) <= (len(terms) + 16.0) * G.U * np.abs(terms).sum()
    g.update(None, S, 0)
    g.end()


# ---------------------------------------------------------------------------------------------------- whole alignment
@pytest.fixture(scope="module")
def scene_ref(api):
    c = GC6.scene()
    ls, lt = GC6.scene_lab(api.lab_tables())
    return c, R.gicp6d(c.src, c.tgt, ls, lt, c.cov_s, c.cov_t, GC6.SCENE_WEIGHT, None, c.prm, truth=c.truth)


def _scene6(api, ctx, device=False):
    c = GC6.scene()
    g = api.GeneralizedIterativeClosestPoint6D(ctx, lab_weight=GC6.SCENE_WEIGHT)
    g.setMaxCorrespondenceDistance(GC6.SCENE_GATE)
    for k, v in GC.TIGHT.items():
        setattr(g.gparams, k, v)
    s, t = GC6.rgb_cloud(c.src, c.rgba_s), GC6.rgb_cloud(c.tgt, c.rgba_t)
    g.setInputSource(api.DeviceCloud(s, ctx=ctx) if device else s)
    g.setInputTarget(api.DeviceCloud(t, ctx=ctx) if device else t)
    g.setSourceCovariances(c.cov_s)
    g.setTargetCovariances(c.cov_t)
    return g


def test_the_scene_aligns_in_six_dimensions_and_not_in_three(api, ctxs, scene_ref):
    c, ref = scene_ref
    g = _scene6(api, ctxs[0])
    g.align()
    T = g.getFinalTransformation().astype(np.float64)
    d_ref, d_truth = float(np.linalg.norm(T - ref.T.astype(np.float64))), float(np.linalg.norm(T - c.truth))
    print("6-D: %d iterations, %d pairs, |T - T_ref|_F %.3g, |T - truth|_F %.3g (reference: %d iterations)"
          % (g.result.iterations, g.result.n_correspondences, d_ref, d_truth, ref.iterations))
    assert g.hasConverged() and g.result.n_correspondences == len(c.src)
    assert d_ref < 1e-4
    assert d_truth < 1e-3
    g3 = api.GeneralizedIterativeClosestPoint(ctxs[0])
    g3.setMaxCorrespondenceDistance(GC6.SCENE_GATE)
    for k, v in GC.TIGHT.items():
        setattr(g3.gparams, k, v)
    g3.setInputSource(GC6.rgb_cloud(c.src, c.rgba_s))
    g3.setInputTarget(GC6.rgb_cloud(c.tgt, c.rgba_t))
    g3.setSourceCovariances(c.cov_s)
    g3.setTargetCovariances(c.cov_t)
    g3.align()
    d3 = float(np.linalg.norm(g3.getFinalTransformation().astype(np.float64) - c.truth))
    print("3-D on the same clouds: |T - truth|_F %.3g" % d3)
    assert g3.hasConverged() and d3 > 5e-3


def test_align_align_cloud_stepwise_and_a_second_context_agree(api, ctxs):
    g = _scene6(api, ctxs[0])
    g.align()
    want = bytes(g.result.transform)
    counts = (g.result.iterations, g.result.inner_evaluations, g.result.n_correspondences)
    gd = _scene6(api, ctxs[0], device=True)
    out = gd.align()
    assert bytes(gd.result.transform) == want and (gd.result.iterations, gd.result.inner_evaluations, gd.result.n_correspondences) == counts
    assert len(out) == len(GC6.scene().src)
    gs = _scene6(api, ctxs[0])
    res = GC.engine_stepwise_align(api, gs)
    assert bytes(res.transform) == want and (res.iterations, res.inner_evaluations, res.n_correspondences) == counts
    g2 = _scene6(api, ctxs[1])
    g2.align()
    assert bytes(g2.result.transform) == want


# ---------------------------------------------------------------------------------------------------- state
def test_state_and_refusals(api, ctxs, boxes):
    from rsreg_amd import lib
    import ctypes as C
    L, h = lib.lib(), ctxs[0].h
    src, lab_s, tgt, lab_t = boxes
    prm = api.gicp_params(max_correspondence_distance=GATE)
    g3 = GC.make_gicp(api, ctxs[0], src, tgt, _unit_cov(len(src)), _unit_cov(len(tgt)), GATE)
    g3.begin()   # clouds and covariances are the context's; no colours yet
    g3.end()
    assert L.rsreg_gicp6d_begin(h, None, C.byref(prm), 0.032) == lib.RSREG_ERR_STATE
    ls, lt = np.ascontiguousarray(lab_s), np.ascontiguousarray(lab_t)
    assert L.rsreg_gicp_set_source_lab(h, ls.ctypes.data, len(ls), 12) == 0
    assert L.rsreg_gicp6d_begin(h, None, C.byref(prm), 0.032) == lib.RSREG_ERR_STATE      # the target's are missing
    assert L.rsreg_gicp_set_target_lab(h, lt.ctypes.data, len(lt) - 1, 12) == lib.RSREG_ERR_INVALID_ARG
    assert L.rsreg_gicp_set_source_lab(h, ls.ctypes.data, len(ls) + 1, 12) == lib.RSREG_ERR_INVALID_ARG
    assert L.rsreg_gicp_set_target_lab(h, lt.ctypes.data, len(lt), 8) == lib.RSREG_ERR_INVALID_ARG
    assert L.rsreg_gicp_set_target_lab(h, lt.ctypes.data, len(lt), 12) == 0
    for bad in (float("nan"), float("inf"), -0.5):
        assert L.rsreg_gicp6d_begin(h, None, C.byref(prm), bad) == lib.RSREG_ERR_INVALID_ARG
    assert L.rsreg_gicp6d_begin(h, None, C.byref(prm), 1.0) == 0
    idx6, d6 = g3.search()
    assert L.rsreg_gicp_end(h, None, None, 0) == 0
    same(idx6, d6, *R.nearest6(src, R.scaled(lab_s, 1.0), tgt, R.scaled(lab_t, 1.0), GATE))
    # a plain rsreg_gicp_begin afterwards searches in three dimensions again
    g3.begin()
    idx3, d3 = g3.search()
    g3.end()
    same(idx3, d3, *R.nearest6(src, R.scaled(lab_s, 0.0), tgt, R.scaled(lab_t, 0.0), GATE))
    assert (idx3 != idx6).any()
    # a new source drops the source's colours
    s = PC.cloud(src)
    assert L.rsreg_icp_set_source(h, s.points.ctypes.data, len(s.points), 32, 0) == 0
    cov = np.ascontiguousarray(_unit_cov(len(src)))
    assert L.rsreg_gicp_set_source_covariances(h, cov.ctypes.data, len(cov), 48) == 0
    assert L.rsreg_gicp6d_begin(h, None, C.byref(prm), 1.0) == lib.RSREG_ERR_STATE
    ctxs[0].icp_source_owner = None
    ctxs[0].icp_target_owner = None
