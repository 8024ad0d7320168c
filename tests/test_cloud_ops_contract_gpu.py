"""The contract every rsreg_cloud_* operation with an input and an output handle keeps, whatever it computes: one table over
passthrough, sor, radius_outlier_removal, normals, normals_radius, fpfh, integral_normals, voxel_grid, edge_features, filter,
transform and copy, on one organized 32 x 24 frame of 32-byte records and two contexts.

On success the output keeps its id and its version goes up by exactly 1, the input (another handle) keeps both, and the output's
n / stride / width / height / is_dense are what include/rsreg.h says.  On a refusal the status code and the rsreg_last_error
text are the literals below, and the output's version, n and stride are untouched.  A refusal that leaves no message leaves
the context's last message alone: every refusal here is made right after a failure with a known text (SENTINEL), so "no
message" is that literal too.

Refusals of every operation: a null context, an input of another context, an output of another context.  A stride below the
operation's minimum: voxel_grid, edge_features and filter need 20 bytes and get 12-byte records.  The other operations'
minimum is 12 bytes and their stride rule asks for a multiple of 4, and rsreg_cloud_upload refuses both kinds of record
(checked here as well), as does every other way to fill a cloud: no handle can hold records those rules would refuse, so
those rows have no case.
"""
import ctypes as C

import numpy as np
import pytest

import edges_ref

pytestmark = pytest.mark.gpu

W, H, N = 32, 24, 32 * 24
INV = -1                                  # RSREG_ERR_INVALID_ARG
SENTINEL = "PassThrough filters on field 0 (x), 1 (y) or 2 (z)"
FPFH_BYTES = 132                          # pcl::FPFHSignature33
LEAF = (0.04, 0.04, 10.0)                 # the frame's pixels are 0.01 apart, an eighth of a leaf off the leaves' faces
N_LEAVES = (W // 4) * (H // 4)


def _frame():
    from rsreg_amd import POINT_DTYPE
    v, u = np.divmod(np.arange(N), W)
    x, y = 0.005 + 0.01 * u, 0.005 + 0.01 * v
    pts = np.zeros(N, POINT_DTYPE)
    pts["x"], pts["y"] = x, y
    pts["z"] = 1.0 + 0.1 * x + 0.05 * y + 2.0 * (x - 0.16) ** 2 + 1.5 * (y - 0.12) ** 2
    pts["w"] = 1.0
    pts["rgba"] = np.where(u < W // 2, 0xFF000000, 0xFFFFFFFF)   # a black and a white half: one Canny edge down the middle
    return pts


class Env:
    def __init__(self):
        from rsreg_amd import api, lib
        self.L = lib.lib()
        self.frame = _frame()
        self.a, self.b = api.Context(0), api.Context(0)
        self.inp = self.cloud(self.a, self.frame, 32)
        self.thin = self.cloud(self.a, np.ascontiguousarray(self.frame.view(np.float32).reshape(N, 8)[:, :3]), 12)
        self.foreign = self.cloud(self.b, self.frame, 32)
        self.normals = self.cloud(self.a)
        self.ok(self.L.rsreg_cloud_normals(self.a.h, self.inp, 3, None, self.normals))
        vg = lib.VoxelGridParams()
        self.L.rsreg_voxel_grid_params_default(C.byref(vg))
        vg.leaf[:] = LEAF
        self.vg, self.leaf = vg, (C.c_float * 3)(*LEAF)
        self.T = (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.5, -0.25, 2.0, 1)

    def ok(self, rc):
        assert rc == 0, (rc, self.L.rsreg_last_error(self.a.h).decode())

    def cloud(self, ctx, rec=None, stride=32):
        h = C.c_void_p()
        assert self.L.rsreg_cloud_create(ctx.h, C.byref(h)) == 0
        if rec is not None:
            assert self.L.rsreg_cloud_upload(h, rec.ctypes.data, N, stride, W, H, 1) == 0
        return h

    def state(self, h):
        i, v = C.c_uint64(), C.c_uint64()
        n, s = C.c_size_t(), C.c_size_t()
        w, ht, d = C.c_uint32(), C.c_uint32(), C.c_int()
        assert self.L.rsreg_cloud_version(h, C.byref(i), C.byref(v)) == 0
        assert self.L.rsreg_cloud_info(h, C.byref(n), C.byref(s), C.byref(w), C.byref(ht), C.byref(d)) == 0
        return (i.value, v.value), (n.value, s.value, w.value, ht.value, d.value)

    def sentinel(self):
        """leave a known message in context a"""
        scratch = self.cloud(self.a)
        assert self.L.rsreg_cloud_passthrough(self.a.h, self.inp, 7, 0.0, 1.0, 0, 0, scratch) == INV
        assert self.L.rsreg_last_error(self.a.h).decode() == SENTINEL
        self.L.rsreg_cloud_destroy(scratch)


@pytest.fixture(scope="module")
def env():
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    return Env()


def _n_edges(e):
    return len(edges_ref.edge_indices(e.frame, W, H))


def _n_approx(e):
    """ApproximateVoxelGrid's count from the library's sequential host restatement"""
    out, n = np.zeros_like(e.frame), C.c_size_t()
    assert e.L.rsreg_approx_voxel_grid(e.frame.ctypes.data, N, 32, e.leaf, out.ctypes.data, C.byref(n)) == 0
    return n.value


# name: (call(e, ctx, in, out), the output's (n, stride, width, height, is_dense) on the frame; a callable: the count n = width)
OPS = {
    # every z lies between the limits: all records kept; PassThrough's compacted output is dense
    "passthrough": (lambda e, c, i, o: e.L.rsreg_cloud_passthrough(c, i, 2, 0.0, 10.0, 0, 0, o), (N, 32, N, 1, 1)),
    "sor": (lambda e, c, i, o: e.L.rsreg_cloud_sor(c, i, 1, 1e9, 0, o, None), (N, 32, N, 1, 1)),
    "radius_outlier_removal": (lambda e, c, i, o: e.L.rsreg_cloud_radius_outlier_removal(c, i, 0.025, 1, 0, 0, o, None), (N, 32, N, 1, 1)),
    "normals": (lambda e, c, i, o: e.L.rsreg_cloud_normals(c, i, 3, None, o), (N, 32, W, H, 1)),
    "normals_radius": (lambda e, c, i, o: e.L.rsreg_cloud_normals_radius(c, i, 0.025, None, o), (N, 32, W, H, 1)),
    "fpfh": (lambda e, c, i, o: e.L.rsreg_cloud_fpfh(c, i, e.normals, 2, o), (N, FPFH_BYTES, W, H, 1)),
    "integral_normals": (lambda e, c, i, o: e.L.rsreg_cloud_integral_normals(c, i, None, o, None), (N, 32, W, H, 0)),
    "voxel_grid": (lambda e, c, i, o: e.L.rsreg_cloud_voxel_grid(c, i, C.byref(e.vg), o, None), (N_LEAVES, 32, N_LEAVES, 1, 1)),
    "edge_features": (lambda e, c, i, o: e.L.rsreg_cloud_edge_features(c, i, o), (_n_edges, 32, _n_edges, 1, 1)),
    "filter": (lambda e, c, i, o: e.L.rsreg_cloud_filter(c, i, e.leaf, o), (_n_approx, 32, _n_approx, 1, 0)),
    "transform": (lambda e, c, i, o: e.L.rsreg_cloud_transform(c, i, e.T, o), (N, 32, W, H, 1)),
    "copy": (lambda e, c, i, o: e.L.rsreg_cloud_copy(c, i, o), (N, 32, W, H, 1)),
}

# (status, rsreg_last_error) of each refusal, as the library gave them before the operations shared their way in
NO_MESSAGE = (INV, SENTINEL)
COMMON = ("null_context", "foreign_input", "foreign_output")
REFUSALS = {(op, case): NO_MESSAGE for op in OPS for case in COMMON}
REFUSALS.update({
    ("voxel_grid", "thin_stride"): (INV, "records need rgb at byte 16 and a stride that is a multiple of 4"),
    ("edge_features", "thin_stride"): (INV, "edge extraction needs an organized XYZRGB cloud"),
    ("filter", "thin_stride"): NO_MESSAGE,
})


@pytest.mark.parametrize("op", list(OPS))
def test_success(env, op):
    call, want = OPS[op]
    want = tuple(f(env) if callable(f) else f for f in want)
    out = env.cloud(env.a)
    in_before, out_before = env.state(env.inp), env.state(out)
    env.ok(call(env, env.a.h, env.inp, out))
    (oid, over), shape = env.state(out)
    print(op, "version", out_before[0][1], "->", over, "shape", shape)
    assert oid == out_before[0][0] and over == out_before[0][1] + 1
    assert env.state(env.inp) == in_before
    assert shape == want
    assert 0 < shape[0] <= N
    env.L.rsreg_cloud_destroy(out)


@pytest.mark.parametrize("op,case", list(REFUSALS))
def test_refusal(env, op, case):
    call = OPS[op][0]
    ctx = None if case == "null_context" else env.a.h
    inp = {"foreign_input": env.foreign, "thin_stride": env.thin}.get(case, env.inp)
    out = env.foreign if case == "foreign_output" else env.cloud(env.a, env.frame, 32)   # (holds records: n and stride could change)
    before = env.state(out)
    env.sentinel()
    rc = call(env, ctx, inp, out)
    text = env.L.rsreg_last_error(env.a.h).decode()
    print(op, case, rc, repr(text))
    assert (rc, text) == REFUSALS[(op, case)]
    after = env.state(out)
    assert after[0] == before[0] and after[1][:2] == before[1][:2]
    if case != "foreign_output":
        env.L.rsreg_cloud_destroy(out)


def test_upload_refuses_the_strides_the_operations_would(env):
    """why the table has no case for a stride below 12 bytes or one that is not a multiple of 4"""
    h = env.cloud(env.a)
    buf = np.zeros(N * 32, np.uint8)
    for stride in (8, 4, 13, 18, 30):
        for up in (env.L.rsreg_cloud_upload, env.L.rsreg_cloud_upload_async, env.L.rsreg_cloud_upload_deferred):
            assert up(h, buf.ctypes.data, N, stride, W, H, 1) == INV
    assert env.state(h)[0][1] == 0
    env.L.rsreg_cloud_destroy(h)
