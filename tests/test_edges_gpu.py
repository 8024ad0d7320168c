"""GPU: the edge extractor (csrc/edges.hip) against the staged numpy reference (tests/edges_ref.py) and the C oracle on the images
of tests/edges_cases.py -- tile seams and corners, images of a few pixels, every step height around both thresholds, equal
neighbours in the suppression, the direction-class boundaries, record strides, the blocks of the compaction.  Indices and record
bytes, equal; no tolerance anywhere.  tests/test_edges_cpu.py shows what each image reaches."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import edges_cases as E
import edges_ref as R
from voxelgrid_cases import Handle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(rs):
    from rsreg_amd import api, lib as L
    L.build()
    if api.device_count() < 1:
        pytest.fail("no HIP device: the product has no CPU fallback")
    return L


@pytest.fixture(scope="module")
def api(lib):
    from rsreg_amd import api as a
    return a


@pytest.fixture(scope="module")
def ctx(api):
    return api.Context(0)


def raw(a, rows=None):
    """the records as rows of bytes, padding included (numpy's copies and fancy indexing of records leave the padding undefined:
    the rows are picked from the bytes)"""
    a = np.ascontiguousarray(a)
    b = a.view(np.uint8).reshape(len(a), a.dtype.itemsize)
    return b if rows is None else b[rows]


def same_fields(out, pts, idx, name=""):
    """the Python layer's host path copies its result field by field: every field bit for bit, as tests/test_edges.py compares"""
    assert len(out) == len(idx), name
    for f in ("x", "y", "z", "w", "rgba"):
        np.testing.assert_array_equal(out[f].view(np.uint32), pts[f][idx].view(np.uint32), err_msg=name)


def run_host(lib, ctx, pts, w, h, want_indices=True):
    """rsreg_extract_edge_features on records of any stride -> (records, indices or None)"""
    src, before = np.ascontiguousarray(pts), pts.tobytes()
    out = np.zeros(len(src), src.dtype)
    idx = np.full(len(src), -1, np.int32)
    n_out = C.c_size_t(0)
    lib.check(lib.lib().rsreg_extract_edge_features(ctx.h, src.ctypes.data, w, h, src.dtype.itemsize, out.ctypes.data,
                                                    idx.ctypes.data if want_indices else None, C.byref(n_out)), ctx.h)
    assert src.tobytes() == before                     # (the input is read only)
    n = n_out.value
    assert not out[n:].tobytes().strip(b"\0") and (idx[n:] == -1).all()      # nothing written behind the edge points
    return out[:n], (idx[:n] if want_indices else None)


def run_cloud(lib, ctx, pts, w, h, is_dense):
    """rsreg_cloud_edge_features on a device cloud of any stride -> (records, info of the output handle)"""
    cin, cout = Handle(lib, ctx, pts, w, h, is_dense), Handle(lib, ctx)
    lib.check(lib.lib().rsreg_cloud_edge_features(ctx.h, cin.h, cout.h), ctx.h)
    info = cout.info()
    out = cout.download(pts.dtype)
    assert cin.info() == (len(pts), pts.dtype.itemsize, w, h, is_dense)
    cin.close()
    cout.close()
    return out, info


def check(name, pts, out, idx):
    want = E.indices(name)
    if idx is not None:
        np.testing.assert_array_equal(idx, want, err_msg=name)
    assert len(out) == len(want), name
    np.testing.assert_array_equal(raw(out), raw(pts, want), err_msg=name)


@pytest.mark.parametrize("group", E.GROUPS)
def test_host_records_equal_reference_and_oracle(rs, lib, api, ctx, orc, group):
    for k, name in enumerate(E.names(group)):
        pts, w, h = E.build(name)
        if pts.dtype == rs.POINT_DTYPE:
            dense = bool(k % 2)
            out, idx = api.extract_edge_features(rs.PointCloud(pts, width=w, height=h, is_dense=dense), ctx, want_indices=True)
            assert (out.width, out.height, out.is_dense) == (len(idx), 1, dense), name
            np.testing.assert_array_equal(idx, E.indices(name), err_msg=name)
            same_fields(out.points, pts, idx, name)
        out, idx = run_host(lib, ctx, pts, w, h)           # the C entry point itself: every byte of the record
        check(name, pts, out, idx)
        np.testing.assert_array_equal(idx, orc.edge_features(pts, w, h), err_msg=name)


@pytest.mark.parametrize("group", E.GROUPS)
def test_device_clouds_equal_reference(lib, ctx, group):
    """rsreg_cloud_edge_features through the C ABI (records of 20, 32 and 48 bytes): the records and the output handle's info"""
    for k, name in enumerate(E.names(group)):
        pts, w, h = E.build(name)
        dense = k % 2
        out, info = run_cloud(lib, ctx, pts, w, h, dense)
        n = len(E.indices(name))
        assert info == (n, pts.dtype.itemsize, n, 1, dense), name
        check(name, pts, out, None)


def test_without_indices(lib, ctx):
    """rsreg_extract_edge_features with indices_out = NULL, at every stride"""
    for name in ("shape_97x70", "records_stride20", "records_stride48", "shape_5x5", "compaction_flat", "compaction_first_and_last"):
        pts, w, h = E.build(name)
        out, _ = run_host(lib, ctx, pts, w, h, want_indices=False)
        check(name, pts, out, None)


def test_every_step_height(lib, ctx, orc):
    """a 12 x 8 step of every height 0..255 in four orientations, one context: empty below the height at which the largest
    magnitude reaches 100 (tests/test_edges_cpu.py: heights on both sides of 40 and of 100 are among them), the reference's
    points from there on"""
    for o in E.THRESHOLD_ORIENTATIONS:
        sweep = E.threshold_sweep(o)
        for delta in range(256):
            pts, w, h = E.threshold_step(o, delta)
            out, idx = run_host(lib, ctx, pts, w, h)
            want = R.edge_indices(pts, w, h)
            np.testing.assert_array_equal(idx, want, err_msg="%s %d" % (o, delta))
            assert len(idx) == sweep[delta][1]
            np.testing.assert_array_equal(raw(out), raw(pts, want))
        first = E.just(o)["strong"]
        np.testing.assert_array_equal(orc.edge_features(E.threshold_step(o, first)[0], 12, 8), R.edge_indices(E.threshold_step(o, first)[0], 12, 8))


def test_strides_alpha_and_geometry_do_not_matter(lib, ctx):
    """the same colours in records of 20, 32 and 48 bytes, under random alpha bytes and non-finite geometry: the same indices;
    contrast in r only and in b only: the same indices; contrast in alpha or in x only: none"""
    base = run_host(lib, ctx, *E.build("shape_97x70"))[1]
    assert len(base) > 1000
    for name in ("records_stride20", "records_stride48", "records_alpha", "records_non_finite", "records_non_finite_stride20"):
        np.testing.assert_array_equal(run_host(lib, ctx, *E.build(name))[1], base, err_msg=name)
    r, b = run_host(lib, ctx, *E.build("records_only_r"))[1], run_host(lib, ctx, *E.build("records_only_b"))[1]
    assert len(r) > 0
    np.testing.assert_array_equal(r, b)
    for name in ("records_only_alpha", "records_only_x"):
        assert len(run_host(lib, ctx, *E.build(name))[1]) == 0, name


def test_async_equals_synchronous(rs, api, ctx):
    """extract_edge_features_async: the side set's scratch and stream"""
    for name in E.names("shapes", "seams"):
        pts, w, h = E.build(name)
        dev = api.DeviceCloud(rs.PointCloud(pts, width=w, height=h, is_dense=False), ctx)
        a = api.extract_edge_features_async(dev)
        got = a.download()
        s = api.extract_edge_features(dev)
        sync = s.download()
        n = len(E.indices(name))
        assert a.info() == (n, 32, n, 1, False), name
        np.testing.assert_array_equal(raw(got.points), raw(sync.points), err_msg=name)
        check(name, pts, got.points, None)
        for d in (a, s, dev):
            d.close()


def test_one_context_many_images(rs, lib, api, ctx):
    """a 640 x 480 frame, then images of a few pixels, flat ones and dense ones through the same scratch: labels, strong flags
    and look-back words of the larger image lie behind the smaller one's"""
    frame = rs.synth.render_frame(0, "N300", "bench")
    want_frame = R.edge_indices(frame.points, frame.width, frame.height)
    assert 0.02 * len(frame) < len(want_frame) < 0.4 * len(frame)
    other = api.Context(0)
    for c in (ctx, other, ctx):
        out, idx = api.extract_edge_features(frame, c, want_indices=True)
        np.testing.assert_array_equal(idx, want_frame)
        same_fields(out.points, frame.points, want_frame, "frame")
        for name in ("shape_5x5", "shape_97x70", "compaction_flat", "compaction_dense", "shape_3x3", "compaction_last", "compaction_first_and_last",
                     "shape_step_3x3", "compaction_first"):
            pts, w, h = E.build(name)
            out, idx = run_host(lib, c, pts, w, h)
            check(name, pts, out, idx)
            out, info = run_cloud(lib, c, pts, w, h, 1)
            check(name, pts, out, None)
    other.close()


def test_repeats_give_the_same_bytes(lib, ctx):
    """the union-find runs concurrently; its result must not depend on the order"""
    for name in E.names("seams") + ["compaction_dense", "shape_97x70", "shape_64x64"]:
        pts, w, h = E.build(name)
        first = None
        for _ in range(3):
            out, idx = run_host(lib, ctx, pts, w, h)
            got = out.tobytes() + idx.tobytes()
            assert first is None or got == first, name
            first = got
        check(name, pts, out, idx)


STAGE_IMAGES = ("shape_97x70", "shape_65x34", "seam_zigzag_last_31_1")

STAGES_CHILD = r'''
import os, shutil, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np
import edges_cases as E
import rsreg_amd as rs
from rsreg_amd import api
ctx = api.Context(0)
for name in %(names)r:
    pts, w, h = E.build(name)
    out, idx = api.extract_edge_features(rs.PointCloud(pts, width=w, height=h, is_dense=False), ctx, want_indices=True)
    np.save(os.path.join(%(out)r, name + "_idx.npy"), idx)
    shutil.copyfile(os.environ["RSREG_EDGE_DUMP"], os.path.join(%(out)r, name + ".bin"))
print("STAGES OK")
'''


def test_stages_equal_reference(lib, tmp_path):
    """The diagnostic build (RSREG_DIAG=1 -> librsreg_diag.so, same sources) dumps the smoothed image, the magnitudes, mx and the
    direction classes (RSREG_EDGE_DUMP), in a child process: all four equal the reference bit for bit.  mx is the product
    kernel's own output (k_edge_tile); the other three come from the stage kernels only the diagnostic build keeps, which
    restate what k_edge_tile computes in LDS -- so they show where a difference in mx begins, not that k_edge_tile is right."""
    lib.build_diag()
    env = dict(os.environ, RSREG_DIAG="1", RSREG_EDGE_DUMP=str(tmp_path / "dump.bin"))
    env.pop("RSREG_SO", None)
    script = STAGES_CHILD % {"root": ROOT, "names": STAGE_IMAGES, "out": str(tmp_path)}
    r = subprocess.run([sys.executable, "-c", script], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and "STAGES OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    for name in STAGE_IMAGES:
        s = E.stages(name)
        n = s.w * s.h
        dump = np.fromfile(tmp_path / (name + ".bin"), np.uint8)
        assert len(dump) == 13 * n
        f = dump[:12 * n].view(np.uint32).reshape(3, s.h, s.w)
        for k, stage in enumerate(("sm", "mag", "mx")):
            np.testing.assert_array_equal(f[k], getattr(s, stage).view(np.uint32), err_msg="%s %s" % (name, stage))
        np.testing.assert_array_equal(dump[12 * n:].reshape(s.h, s.w), s.dir, err_msg=name)
        np.testing.assert_array_equal(np.load(tmp_path / (name + "_idx.npy")), s.indices)
