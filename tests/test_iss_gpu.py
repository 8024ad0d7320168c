"""rsreg_cloud_iss_saliency, rsreg_cloud_iss_non_max and rsreg_cloud_iss_keypoints (pcl::ISSKeypoint3D) on the GPU, the Python and
C++ adaptors, against tests/iss_ref.py.  The stages are held separately, so that no rounding hides a logic error:

  1. sums and solve: count_out EQUALS the radius search's counts at the salient radius; every eigenvalue is within
     1e-12 * trace_ref of numpy's -- the bound of tests/test_radius_gpu.py (the two scatters differ by the order of their double
     sums, m * 2^-53 of the second moments, m <= 5 000 here; the solves are backward stable to a few 2^-53 of the trace), taken
     from there, not measured; records below min_neighbors and non-finite records hold zeros; the hand case and the lattice, whose
     sums are exact in any order, are held to equality;
  2. threshold: saliency_out EQUALS, bit for bit, the rule applied in numpy to the device's own eigenvalues, on every record;
  3. suppression: iss_non_max over the device's own saliencies EQUALS the reference suppression of the same array on every record,
     and iss_keypoints returns exactly those indices and exactly those records, byte for byte;
  4. end to end against the reference alone: keypoint membership equals the reference's on every record that is not fragile
     (iss_ref.fragile; the share of fragile records is capped on the reference by tests/test_iss_cpu.py);
  5. the shapes that can break a kernel: a non-max radius 2.5 and 0.1 times the salient one over the ONE index built for the
     salient radius, more finite records than a launch has workgroups, every record stride, the float32 range, a radius whose
     square is +inf, one / no finite record, an empty cloud, every refusal, the capacity of the index list, a second context;
  6. the adaptors: api.ISSKeypoint3D from host and device clouds, tests/cpp/iss_runner.cpp through rsreg::ISSKeypoint3D."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import iss_cases as IC
import iss_ref as I
import layout_cases as L
import radius_cases as K
import radius_ref as R
import trips_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
EIG_BOUND = 1e-12


@pytest.fixture(scope="module")
def api():
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    return api


@pytest.fixture(scope="module")
def ctx(api):
    return api.Context(0)


def _records(points, idx):
    return np.ascontiguousarray(points).view(np.uint8).reshape(len(points), -1)[idx].tobytes()


def _stages(api, ctx, cloud, xyz, ref, label, **params):
    """Stages 1 to 3 on one cloud: returns (eig, saliency, counts, indices) of the device."""
    p = dict(gamma_21=0.975, gamma_32=0.975, min_neighbors=5)
    p.update(params)
    dc = api.DeviceCloud(cloud, ctx=ctx)
    eig, sal, m = dc.iss_saliency(**p)
    assert eig.shape == (len(xyz), 3) and eig.dtype == np.float64 and sal.dtype == np.float64 and m.dtype == np.uint32
    # 1
    np.testing.assert_array_equal(m, ref.nb_s.counts())
    slack = (np.abs(eig - ref.eig) - EIG_BOUND * ref.trace[:, None]).max() if len(xyz) else 0.0
    assert (np.diff(eig, axis=1) >= 0).all()
    assert (eig[m < p["min_neighbors"]] == 0).all() and (eig[~ref.nb_s.fin] == 0).all()
    # 2
    want = I.saliency_rule(eig, p["gamma_21"], p["gamma_32"])
    # 3
    key = I.non_max(sal, ref.nb_n, p["min_neighbors"])
    got = dc.iss_non_max(sal, p["non_max_radius"], p["min_neighbors"])
    out, idx = dc.iss_keypoints(**p)
    kp = out.info()
    print("iss %s: n %d, m_s %d .. %d, eigenvalue slack %.3g, salient %d, keypoints %d, saliency rows that differ %d, suppression rows that differ %d" %
          (label, len(xyz), m.min() if len(m) else 0, m.max() if len(m) else 0, slack, int((sal > 0).sum()), len(idx),
           int((sal.view(np.uint64) != want.view(np.uint64)).sum()), int((got != key).sum())))
    assert slack <= 0
    assert sal.tobytes() == want.tobytes()
    np.testing.assert_array_equal(got, key)
    assert idx.dtype == np.int32 and idx.tolist() == np.flatnonzero(key).tolist()
    assert kp == (len(idx), kp[1], len(idx), 1, True)
    return eig, sal, m, idx, out


# ------------------------------------------------------------------------------------------------ stages 1 to 4, every case
@pytest.mark.parametrize("name,salient,non_max", IC.CASES)
def test_stages_against_the_reference(api, ctx, name, salient, non_max):
    cloud = K.input_cloud(name)
    ref = IC.reference(name, salient, non_max)
    eig, sal, m, idx, out = _stages(api, ctx, cloud, cloud.xyz, ref, "%s %g / %g" % (name, salient, non_max), salient_radius=salient, non_max_radius=non_max)
    np.testing.assert_array_equal(m, api.DeviceCloud(cloud, ctx=ctx).radius_count(salient))
    assert out.download().points.tobytes() == _records(cloud.points, idx)
    # 4: against the reference alone, on the records whose membership the eigenvalue bound cannot move
    key = np.zeros(len(cloud), bool)
    key[idx] = True
    firm = ~IC.fragile(name, salient, non_max)
    differ = int((key != ref.keypoint)[firm].sum())
    print("    end to end: reference keypoints %d, firm records %d of %d, firm records that differ %d, all that differ %d" %
          (len(ref.indices), int(firm.sum()), len(cloud), differ, int((key != ref.keypoint).sum())))
    assert differ == 0
    if name.startswith("lattice"):
        # every sum is exact: a diagonal scatter gives its diagonal, bit for bit, and the scatter's trace whatever the solve did
        diag = (ref.S == ref.S * np.eye(3)).all(axis=(1, 2)) & (m >= 5)
        assert diag.sum() > 1000
        assert (eig[diag] == np.sort(np.diagonal(ref.S, axis1=1, axis2=2)[diag], axis=1)).all()
        assert (eig[IC.INNER] == 10 * K.H ** 2).all()
        assert (np.abs(eig.sum(axis=1) - ref.trace) <= EIG_BOUND * ref.trace).all()
        corners = [(x * 12 + y) * 12 + z for x in (0, 11) for y in (0, 11) for z in (0, 11)]      # mirror images of each other:
        assert m[corners].tolist() == [7] * 8 and len({eig[c].tobytes() for c in corners}) == 1   # the same bits, rotations included
    else:
        counts = {("sphere5000", 0.1): 277, ("uniform5000", 0.1): 108, ("uniform1000", 0.2): 46, ("non_finite", 0.15): 258,
                  ("frame_pass", 0.06): 2281, ("frame_pass", 0.03): 2344, ("frame_raw", 0.06): 2281}
        assert len(ref.indices) == counts[(name, salient)]       # (the reference's own: what the case is)


def test_hand_case(api, ctx):
    cloud, xyz, r, mn = IC.hand_cloud(), IC.hand_xyz(), IC.HAND_RADIUS, IC.HAND_MIN_NEIGHBORS
    ref = I.detect(xyz, r, r, min_neighbors=mn)
    eig, sal, m, idx, _ = _stages(api, ctx, cloud, xyz, ref, "hand", salient_radius=r, non_max_radius=r, min_neighbors=mn)
    assert m.tolist() == [7, 2, 2, 5, 5, 5, 5]
    assert tuple(eig[0]) == IC.HAND_EIG and (eig[1:] == 0).all()
    assert sal.tolist() == [2.0 ** -9] + [0.0] * 6 and idx.tolist() == [0]
    dc = api.DeviceCloud(cloud, ctx=ctx)
    assert len(dc.iss_keypoints(salient_radius=r, non_max_radius=r, min_neighbors=mn, gamma_21=0.25)[1]) == 0          # 0.25 < 0.25 fails
    assert dc.iss_keypoints(salient_radius=r, non_max_radius=r, min_neighbors=mn, gamma_21=float(np.nextafter(0.25, 1)))[1].tolist() == [0]
    assert len(dc.iss_keypoints(salient_radius=r, non_max_radius=r, min_neighbors=mn, gamma_32=0.25)[1]) == 0
    assert len(dc.iss_keypoints(salient_radius=r, non_max_radius=r, min_neighbors=8)[1]) == 0


# ------------------------------------------------------------------------------------------------ 3: planted saliencies
def test_planted_saliencies(api, ctx):
    n = 12 ** 3
    dc = api.DeviceCloud(K.input_cloud("lattice"), ctx=ctx)
    i, f = IC.INNER, IC.FACE

    def run(s, radius, mn, name="lattice", on=None):
        got = (on or dc).iss_non_max(s, radius, mn)
        np.testing.assert_array_equal(got, I.non_max(s, IC.search(name, radius), mn))
        return got

    both = run(IC.planted(n, **{"i%d" % i: 1.0, "i%d" % f: 1.0}), K.R_FACE, 5)                # a tie: both stay
    assert both[i] and both[f] and both.sum() == 2
    at = run(IC.planted(n, **{"i%d" % i: 1.0, "i%d" % f: 2.0}), K.R_AT, 1)                     # the larger one AT the radius: no neighbour
    assert at[i] and at[f] and at.sum() == 2
    inside = run(IC.planted(n, **{"i%d" % i: 1.0, "i%d" % f: 2.0}), K.R_FACE, 5)               # just inside: suppressed
    assert not inside[i] and inside[f] and inside.sum() == 1
    odd = IC.planted(n, **{"i%d" % i: 1.0, "i%d" % f: np.nan, "i%d" % (i - 144): -1.0, "i%d" % (i + 12): 0.0, "i%d" % (i - 12): -np.inf})
    got = run(odd, K.R_FACE, 5)                                                              # NaN, negative, zero: never keypoints, suppress nothing
    assert got[i] and got.sum() == 1
    far = i + 3 * 144
    inf = IC.planted(n, **{"i%d" % far: np.inf, "i%d" % (far + 1): np.inf, "i%d" % (far - 1): 1e300, "i%d" % (far + 12): 1.0})
    got = run(inf, K.R_FACE, 5)                                                              # +inf: a keypoint, ties with +inf, suppresses the rest
    assert got[far] and got[far + 1] and not got[far - 1] and not got[far + 12] and got.sum() == 2
    one = IC.planted(n, **{"i%d" % i: 1.0})                                                  # m_n = 7
    assert run(one, K.R_FACE, 6)[i] and run(one, K.R_FACE, 7)[i] and not run(one, K.R_FACE, 8).any()
    assert run(one, K.R_FACE, 0)[i] and not run(np.zeros(n), K.R_FACE, 0).any()
    # the pile: point 777 and its 300 copies, one cell's run longer than a wave -- equal values: all keypoints or none
    pile_dc = api.DeviceCloud(K.input_cloud("lattice_pile"), ctx=ctx)
    pile = np.r_[777, 1728:2028]
    s = np.zeros(2028)
    s[pile] = 3.0
    got = run(s, K.R_FACE, 5, "lattice_pile", pile_dc)
    assert got[pile].all() and got.sum() == 301
    s[777 + 144] = 4.0
    got = run(s, K.R_FACE, 5, "lattice_pile", pile_dc)
    assert not got[pile].any() and got[777 + 144] and got.sum() == 1


# ------------------------------------------------------------------------------------------------ 5: shapes
@pytest.mark.parametrize("name,salient,factor,mn", [("uniform5000", 0.1, 2.5, 5), ("uniform5000", 0.1, 0.1, 1), ("sphere5000", 0.1, 2.5, 5),
                                                    ("sphere5000", 0.1, 0.1, 1), ("lattice_pile", K.R_FACE, 2.5, 5)])
def test_non_max_radius_above_and_below_the_cell(api, ctx, name, salient, factor, mn):
    """iss_keypoints walks the index built for the salient radius with the other radius: reach 2.5 cells and more, and 0.1 cell."""
    cloud = K.input_cloud(name)
    non_max = salient * factor
    ref = I.detect(cloud.xyz, salient, non_max, min_neighbors=mn, nb_s=IC.search(name, salient), nb_n=IC.search(name, non_max))
    eig, sal, m, idx, _ = _stages(api, ctx, cloud, cloud.xyz, ref, "%s %g x %g" % (name, salient, factor), salient_radius=salient, non_max_radius=non_max,
                                  min_neighbors=mn)
    assert ref.m_n.max() >= mn and (name == "lattice_pile" or len(idx) > 0)
    if factor > 1:
        assert ref.m_n.max() > ref.m_s.max()


def test_more_records_than_workgroups(api, ctx):
    """65 537 finite records and 1 500 holes: a workgroup of either kernel answers a second record, record ids pass 65 535."""
    xyz, cloud = T.xyz("launch_edge_65537"), T.cloud("launch_edge_65537")
    ref = I.detect(xyz, 0.05, 0.03)
    eig, sal, m, idx, out = _stages(api, ctx, cloud, xyz, ref, "launch_edge_65537", salient_radius=0.05, non_max_radius=0.03)
    assert int(np.isfinite(xyz).all(axis=1).sum()) == 65537 > T.LAUNCH_CAP and idx.max() > 65535 and len(idx) > 100
    assert out.download().points.tobytes() == _records(cloud.points, idx)


def test_every_stride(api, ctx):
    from rsreg_amd import lib
    xyz = L.non_finite_xyz()
    ref = IC.reference("non_finite", 0.15, 0.1)
    base = None
    for stride in L.STRIDES:
        raw = L.raw_cloud(xyz, stride, 60, 50)
        dc = api.DeviceCloud(raw, ctx=ctx)
        eig, sal, m = dc.iss_saliency(salient_radius=0.15, non_max_radius=0.1)
        out, idx = dc.iss_keypoints(salient_radius=0.15, non_max_radius=0.1)
        assert out.info() == (len(idx), stride, len(idx), 1, True)
        buf = np.zeros((len(idx), stride // 4), np.uint32)
        lib.check(lib.lib().rsreg_cloud_download(out.h, buf.ctypes.data, len(idx)), ctx.h)
        assert buf.tobytes() == L.as_words(raw.points)[idx].tobytes()
        got = (eig.tobytes(), sal.tobytes(), m.tobytes(), idx.tobytes())
        base = base or got
        assert got == base
    assert (np.abs(np.frombuffer(base[0]).reshape(-1, 3) - ref.eig) <= EIG_BOUND * ref.trace[:, None]).all() and len(np.frombuffer(base[3], np.int32)) > 100


@pytest.mark.parametrize("shift", [20, -20])
def test_float32_range(api, ctx, shift):
    """The cloud and both radii times 2^shift: every product is the scale-1 product times a power of two, so the indices are the same
    and the eigenvalues are the scale-1 bytes moved by 2^(2 shift)."""
    name, salient, non_max = "uniform1000", 0.2, 0.12
    xyz = K.input_cloud(name).xyz
    s = 2.0 ** shift
    base = api.DeviceCloud(K.cloud(xyz), ctx=ctx)
    moved = api.DeviceCloud(K.cloud(xyz * np.float32(s)), ctx=ctx)
    e0, s0, m0 = base.iss_saliency(salient_radius=salient, non_max_radius=non_max)
    e1, s1, m1 = moved.iss_saliency(salient_radius=salient * s, non_max_radius=non_max * s)
    assert (m0 == m1).all() and (e1 == e0 * s * s).all() and (s1 == s0 * s * s).all() and (s0 > 0).sum() > 100
    i0, i1 = base.iss_keypoints(salient_radius=salient, non_max_radius=non_max)[1], moved.iss_keypoints(salient_radius=salient * s, non_max_radius=non_max * s)[1]
    assert i0.tolist() == i1.tolist() == IC.reference(name, salient, non_max).indices.tolist()


def test_huge_radius_and_small_clouds(api, ctx):
    name = "uniform1000"
    cloud = K.input_cloud(name)
    everyone = R.search(cloud.xyz, 10.0)                       # the ball holds the cloud, as the one of 1e30 does (r * r = +inf as a float)
    assert (everyone.counts() == 1000).all()
    ref = I.detect(cloud.xyz, 10.0, 0.12, nb_s=everyone, nb_n=IC.search(name, 0.12))
    eig, sal, m, idx, _ = _stages(api, ctx, cloud, cloud.xyz, ref, "uniform1000 salient 1e30", salient_radius=1e30, non_max_radius=0.12)
    assert (m == 1000).all() and len(idx) >= 1
    for small, n in (("one", 9), ("none_finite", 70), ("empty", 0)):
        c = K.input_cloud(small)
        ref = I.detect(c.xyz, 0.5, 0.3, min_neighbors=0)
        eig, sal, m, idx, out = _stages(api, ctx, c, c.xyz, ref, small, salient_radius=0.5, non_max_radius=0.3, min_neighbors=0)
        assert len(eig) == n and len(idx) == 0 and (eig == 0).all() and len(out) == 0     # (one record: a zero scatter, saliency 0)
        assert m.sum() == (1 if small == "one" else 0)
    dc = api.DeviceCloud(cloud, ctx=ctx)                       # ... and the context goes on
    assert dc.iss_keypoints(salient_radius=0.2, non_max_radius=0.12)[1].tolist() == IC.reference(name, 0.2, 0.12).indices.tolist()


def test_refusals_leave_out_unchanged(api, ctx):
    from rsreg_amd import lib
    Lh = lib.lib()
    inv = lib.RSREG_ERR_INVALID_ARG
    dc = api.DeviceCloud(K.cloud(K.uniform(40, 8)), ctx=ctx)
    out = api.DeviceCloud(K.cloud(K.uniform(7, 9)), ctx=ctx)
    before, stamp = out.download().points.tobytes(), out.stamp
    idx = np.full(40, -7, np.int32)
    found = C.c_uint64(99)
    eig, sal, m, flags = np.full(120, 7.0), np.full(40, 7.0), np.full(40, 77, np.uint32), np.full(40, 9, np.uint8)

    def keypoints(p, cin=dc, cout=out):
        return Lh.rsreg_cloud_iss_keypoints(ctx.h, cin.h if cin is not None else None, C.byref(p) if p is not None else None, cout.h if cout is not None else None, idx.ctypes.data, 40, C.byref(found))

    def saliency(p, cin=dc):
        return Lh.rsreg_cloud_iss_saliency(ctx.h, cin.h if cin is not None else None, C.byref(p) if p is not None else None, eig.ctypes.data, sal.ctypes.data, m.ctypes.data)

    good = dict(salient_radius=0.3, non_max_radius=0.2)
    for bad in (0.0, -0.03, float("nan"), float("inf"), float("-inf")):
        assert keypoints(api.iss_params(**dict(good, salient_radius=bad))) == inv
        assert keypoints(api.iss_params(**dict(good, non_max_radius=bad))) == inv
        assert saliency(api.iss_params(**dict(good, salient_radius=bad))) == inv
        assert Lh.rsreg_cloud_iss_non_max(ctx.h, dc.h, sal.ctypes.data, bad, 5, flags.ctypes.data) == inv
    assert keypoints(api.iss_params(non_max_radius=0.2)) == inv and keypoints(api.iss_params(salient_radius=0.3)) == inv    # the defaults: radii 0
    for field in ("gamma_21", "gamma_32"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert keypoints(api.iss_params(**dict(good, **{field: bad}))) == inv
            assert saliency(api.iss_params(**dict(good, **{field: bad}))) == inv
    assert keypoints(api.iss_params(**dict(good, min_neighbors=-1))) == inv
    assert saliency(api.iss_params(**dict(good, min_neighbors=-1))) == inv
    assert Lh.rsreg_cloud_iss_non_max(ctx.h, dc.h, sal.ctypes.data, 0.2, -1, flags.ctypes.data) == inv
    ok = api.iss_params(**good)
    assert keypoints(ok, cout=dc) == inv                                                       # out == in
    assert keypoints(ok, cin=None) == inv and keypoints(None) == inv and saliency(ok, cin=None) == inv and saliency(None) == inv
    assert Lh.rsreg_cloud_iss_non_max(ctx.h, None, sal.ctypes.data, 0.2, 5, flags.ctypes.data) == inv
    assert Lh.rsreg_cloud_iss_non_max(ctx.h, dc.h, None, 0.2, 5, flags.ctypes.data) == inv
    assert Lh.rsreg_cloud_iss_non_max(ctx.h, dc.h, sal.ctypes.data, 0.2, 5, None) == inv
    other = api.Context(0)
    foreign_in, foreign_out = api.DeviceCloud(K.cloud(K.uniform(40, 8)), ctx=other), api.DeviceCloud(ctx=other)
    assert keypoints(ok, cin=foreign_in) == inv and keypoints(ok, cout=foreign_out) == inv and saliency(ok, cin=foreign_in) == inv
    assert Lh.rsreg_cloud_iss_non_max(ctx.h, foreign_in.h, sal.ctypes.data, 0.2, 5, flags.ctypes.data) == inv
    assert out.download().points.tobytes() == before and out.stamp == stamp and len(dc) == 40 and len(foreign_out) == 0
    assert (idx == -7).all() and found.value == 99 and (eig == 7).all() and (sal == 7).all() and (m == 77).all() and (flags == 9).all()
    with pytest.raises(lib.RsregError) as e:
        dc.iss_keypoints(salient_radius=0.3)
    assert e.value.status == inv
    lib.check(keypoints(ok), ctx.h)                                                            # ... and the call that is right
    assert out.stamp[1] != stamp[1] and found.value == len(out) and (idx[:found.value] >= 0).all() and (idx[found.value:] == -7).all()


def test_capacity_and_nullable_outputs(api, ctx):
    from rsreg_amd import lib
    Lh = lib.lib()
    name, salient, non_max = "uniform1000", 0.2, 0.12
    cloud = K.input_cloud(name)
    dc = api.DeviceCloud(cloud, ctx=ctx)
    want = dc.iss_keypoints(salient_radius=salient, non_max_radius=non_max)[1]
    k = len(want)
    p = api.iss_params(salient_radius=salient, non_max_radius=non_max)
    for cap in (0, 1, k - 1, k, k + 1, 1000):
        idx = np.full(1001, -7, np.int32)
        found = C.c_uint64(0)
        lib.check(Lh.rsreg_cloud_iss_keypoints(ctx.h, dc.h, C.byref(p), None, idx.ctypes.data, cap, C.byref(found)), ctx.h)   # out may be NULL
        assert found.value == k and idx[:min(cap, k)].tolist() == want[:cap].tolist() and (idx[min(cap, k):] == -7).all()
    out = api.DeviceCloud(ctx=ctx)
    found = C.c_uint64(0)
    lib.check(Lh.rsreg_cloud_iss_keypoints(ctx.h, dc.h, C.byref(p), out.h, None, 0, C.byref(found)), ctx.h)                  # index_out may be NULL
    assert found.value == k and out.download().points.tobytes() == _records(cloud.points, want)
    lib.check(Lh.rsreg_cloud_iss_keypoints(ctx.h, dc.h, C.byref(p), out.h, None, 0, None), ctx.h)                            # ... and n_keypoints
    assert len(out) == k
    sal = np.zeros(1000)
    lib.check(Lh.rsreg_cloud_iss_saliency(ctx.h, dc.h, C.byref(p), None, sal.ctypes.data, None), ctx.h)                      # eig_out, count_out
    assert sal.tobytes() == dc.iss_saliency(salient_radius=salient, non_max_radius=non_max)[1].tobytes()
    lib.check(Lh.rsreg_cloud_iss_saliency(ctx.h, dc.h, C.byref(p), None, None, None), ctx.h)


def test_same_bytes_from_a_second_context(api, ctx):
    """The piles (300 copies in one cell, the raw frame's 6 558) are where an order left to the build would show in the last bits."""
    for name, salient, non_max in (("lattice_pile", K.R_EDGE, K.R_FACE), ("frame_raw", 0.06, 0.04), ("sphere5000", 0.1, 0.06)):
        cloud = K.input_cloud(name)
        p = dict(salient_radius=salient, non_max_radius=non_max)
        dc = api.DeviceCloud(cloud, ctx=ctx)
        first = [a.tobytes() for a in dc.iss_saliency(**p)] + [dc.iss_keypoints(**p)[1].tobytes()]
        again = [a.tobytes() for a in dc.iss_saliency(**p)] + [dc.iss_keypoints(**p)[1].tobytes()]
        other = api.Context(0)                                  # a context that has searched other clouds first
        api.DeviceCloud(K.input_cloud("uniform5000"), ctx=other).normals_radius(0.05)
        api.DeviceCloud(K.input_cloud("sphere5000"), ctx=other).radius_count(0.2)
        fresh_dc = api.DeviceCloud(cloud, ctx=other)
        fresh_out, fresh_idx = fresh_dc.iss_keypoints(**p)
        fresh = [a.tobytes() for a in fresh_dc.iss_saliency(**p)] + [fresh_idx.tobytes()]
        assert first == again == fresh
        assert fresh_out.download().points.tobytes() == _records(cloud.points, fresh_idx)


# ------------------------------------------------------------------------------------------------ 6: adaptors
def test_adaptors(api, ctx, tmp_path):
    name, salient, non_max = "frame_raw", 0.06, 0.04
    fr = K.input_cloud(name)
    dc = api.DeviceCloud(fr, ctx=ctx)
    want_out, want = dc.iss_keypoints(salient_radius=salient, non_max_radius=non_max)
    want_rec = want_out.download().points.tobytes()
    assert len(want) > 1000 and want_rec == _records(fr.points, want)
    iss = api.ISSKeypoint3D()
    iss.setSalientRadius(salient)
    iss.setNonMaxRadius(non_max)
    iss.setInputCloud(fr)                                       # a host cloud: through a temporary DeviceCloud
    host = iss.compute()
    assert host.points.tobytes() == want_rec and (host.width, host.height, host.is_dense) == (len(want), 1, True)
    assert iss.getKeypointsIndices().tolist() == want.tolist()
    iss.setInputCloud(dc)
    dev = iss.compute()
    assert isinstance(dev, api.DeviceCloud) and dev.download().points.tobytes() == want_rec and iss.getKeypointsIndices().tolist() == want.tolist()
    iss.setThreshold21(0.8)
    iss.setThreshold32(0.7)
    iss.setMinNeighbors(20)
    tight = iss.compute()
    assert iss.getKeypointsIndices().tolist() == dc.iss_keypoints(salient_radius=salient, non_max_radius=non_max, gamma_21=0.8, gamma_32=0.7,
                                                                   min_neighbors=20)[1].tolist() != want.tolist() and len(tight) > 0

    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "iss_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "iss_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    fr.points.tofile(str(tmp_path / "in.bin"))
    names = ["idx_host.bin", "idx_dev.bin", "kp_host.bin", "kp_dev.bin"]
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(fr.width), str(fr.height), repr(salient), repr(non_max), "0.975", "0.975", "5"] +
                       [str(tmp_path / f) for f in names], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    vals = dict(l.split() for l in r.stdout.strip().splitlines())
    for f in names[:2]:
        assert open(str(tmp_path / f), "rb").read() == want.tobytes()          # the indices of the C call
    for f in names[2:]:
        assert open(str(tmp_path / f), "rb").read() == want_rec
    assert int(vals["size"]) == int(vals["size_device"]) == int(vals["indices"]) == int(vals["indices_device"]) == int(vals["width"]) == len(want)
    assert vals["height"] == "1" and vals["dense"] == vals["dense_device"] == "1" and vals["border_refused"] == "yes"
