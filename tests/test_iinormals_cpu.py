"""CPU: the reference of IntegralImageNormalEstimation (tests/iinormals_ref.py) on inputs whose answer is known without it, and
the host side of the new entry points."""
import os
import subprocess

import numpy as np

import iinormals_cases as K
import iinormals_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plane_normals_face_the_viewpoint():
    a, b, c = 0.25, -0.5, 2.0
    P = K.plane_frame(64, 48, a, b, c)
    want = np.array([a, b, -1.0]) / np.sqrt(a * a + b * b + 1.0)      # the side of the plane the origin is on
    for vp, sign in (((0.0, 0.0, 0.0), 1.0), ((0.0, 0.0, 10.0), -1.0)):
        res = R.normals(P, viewpoint=vp)
        inner = np.zeros((48, 64), bool)
        inner[10:38, 10:54] = True
        assert (res.has_normal == inner.reshape(-1)).all() and (res.rect[res.has_normal] == 10).all()
        n = R.normal_vectors(res.records)[res.has_normal].astype(np.float64)
        assert np.abs(n - sign * want).max() <= 1e-5
        v = np.asarray(vp)[None, :] - P.reshape(-1, 3)[res.has_normal]
        assert ((v * n).sum(axis=1) > 0).all()
        words = res.records
        assert (words[:, [3, 5, 6, 7]] == 0).all() and (words[:, 4] == R.QNAN).all()
        assert (words[~res.has_normal][:, [0, 1, 2]] == R.QNAN).all()


def test_recurrence_and_cumsum_agree_on_a_quantised_cloud():
    P = K.quantised_cloud()
    a, b = R.normals(P, table="cumsum"), R.normals(P, table="recurrence")
    assert a.records.tobytes() == b.records.tobytes() and (a.rect == b.rect).all()
    assert a.has_normal.sum() > 1000 and (a.rect == 0).sum() > 1000 and len(np.unique(a.rect)) >= 8


def _one_zero(r, c, w=12, h=9):
    M = np.ones((h, w), bool)
    M[r, c] = False
    return R.distance_map(M)


def test_distance_map_quirks_by_hand():
    """12 x 9 maps, start value 21, one zero each.  Forward: column 0 is never written and is the last column's "up-right";
    backward: column w-1 and row h-1 are never written and column w-1 is the first column's "lower-left"."""
    # the zero in column 0, row 4: the forward pass hands it to (4, 11) as 0 + 1.4; rows 0 .. 3 of column 11 stay 21 (their
    # "up-right" D[r][0] is still 21 when they are visited, and the backward pass does not write the column); (8, 0) stays 21
    D = _one_zero(4, 0)
    want = np.array([
        [4.0, 4.4, 4.8, 5.2, 5.6, 6.6, 7.6, 7.0, 6.6, 6.2, 5.8, 21.0],
        [3.0, 3.4, 3.8, 4.2, 5.2, 6.2, 7.2, 6.6, 5.6, 5.2, 4.8, 21.0],
        [2.0, 2.4, 2.8, 3.8, 4.8, 5.8, 6.8, 6.2, 5.2, 4.2, 3.8, 21.0],
        [1.0, 1.4, 2.4, 3.4, 4.4, 5.4, 6.4, 5.8, 4.8, 3.8, 2.8, 21.0],
        [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 5.4, 4.4, 3.4, 2.4, 1.4],
        [2.4, 1.4, 2.4, 3.4, 4.4, 5.4, 6.4, 5.8, 4.8, 3.8, 2.8, 2.4],
        [3.4, 2.4, 2.8, 3.8, 4.8, 5.8, 6.8, 6.2, 5.2, 4.2, 3.8, 3.4],
        [4.4, 3.4, 3.8, 4.2, 5.2, 6.2, 7.2, 6.6, 5.6, 5.2, 4.8, 4.4],
        [21.0, 4.4, 4.8, 5.2, 5.6, 6.6, 7.6, 7.0, 6.6, 6.2, 5.8, 5.4]])
    assert np.abs(D - want).max() < 1e-5
    assert D[4, 11] == np.float32(1.4) and D[5, 0] == np.float32(np.float32(1.4) + np.float32(1.0))
    # the zero in column w-1, row 4: the backward pass hands it to (4, 0) as 0 + 1.4, and (5, 11) = 1 to (5, 0) as 2.4; column 0
    # then feeds its right neighbours; row 8 keeps the forward pass's values
    D = _one_zero(4, 11)
    want = np.array([
        [5.4, 5.8, 6.2, 6.6, 7.0, 7.6, 6.6, 5.6, 5.2, 4.8, 4.4, 21.0],
        [4.4, 4.8, 5.2, 5.6, 8.0, 7.2, 6.2, 5.2, 4.2, 3.8, 3.4, 21.0],
        [3.4, 3.8, 4.2, 6.6, 7.8, 6.8, 5.8, 4.8, 3.8, 2.8, 2.4, 21.0],
        [2.4, 2.8, 5.2, 7.6, 7.4, 6.4, 5.4, 4.4, 3.4, 2.4, 1.4, 21.0],
        [1.4, 3.8, 6.2, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0, 0.0],
        [2.4, 4.8, 7.2, 8.4, 7.4, 6.4, 5.4, 4.4, 3.4, 2.4, 1.4, 1.0],
        [3.4, 5.8, 9.8, 8.8, 7.8, 6.8, 5.8, 4.8, 3.8, 2.8, 2.4, 2.0],
        [4.4, 11.2, 10.2, 9.2, 8.2, 7.2, 6.2, 5.2, 4.2, 3.8, 3.4, 3.0],
        [21.0, 21.0, 21.0, 21.0, 21.0, 21.0, 21.0, 5.6, 5.2, 4.8, 4.4, 4.0]])
    assert np.abs(D - want).max() < 1e-5
    assert D[4, 0] == np.float32(1.4)
    # the zero in row 0: the backward pass spreads it along row 0 to the left; to the right the row keeps what the forward
    # pass left: (0, 6) .. (0, 10) come from row 1, (0, 11) stays 21
    D = _one_zero(0, 5)
    want = np.array([
        [5.0, 4.0, 3.0, 2.0, 1.0, 0.0, 2.4, 2.8, 3.8, 4.8, 5.8, 21.0],
        [5.4, 4.4, 3.4, 2.4, 1.4, 1.0, 1.4, 2.4, 3.4, 4.4, 5.4, 6.4],
        [5.8, 4.8, 3.8, 2.8, 2.4, 2.0, 2.4, 2.8, 3.8, 4.8, 5.8, 6.8],
        [6.2, 5.2, 4.2, 3.8, 3.4, 3.0, 3.4, 3.8, 4.2, 5.2, 6.2, 7.2],
        [6.6, 5.6, 5.2, 4.8, 4.4, 4.0, 4.4, 4.8, 5.2, 5.6, 6.6, 7.6],
        [7.6, 6.6, 6.2, 5.8, 5.4, 5.0, 5.4, 5.8, 6.2, 6.6, 7.0, 8.0],
        [8.6, 7.6, 7.2, 6.8, 6.4, 6.0, 6.4, 6.8, 7.2, 7.6, 8.0, 8.4],
        [9.6, 8.6, 8.2, 7.8, 7.4, 7.0, 7.4, 7.8, 8.2, 8.6, 9.0, 9.4],
        [21.0, 9.6, 9.2, 8.8, 8.4, 8.0, 8.4, 8.8, 9.2, 9.6, 10.0, 10.4]])
    assert np.abs(D - want).max() < 1e-5
    # the zero in row h-1: the forward pass spreads it to the right along the row, the backward pass upwards; the row's left
    # part and column 11 above it are never reached
    D = _one_zero(8, 5)
    want = np.array([
        [10.0, 9.6, 9.2, 8.8, 8.4, 8.0, 8.4, 8.8, 9.2, 9.6, 10.0, 21.0],
        [9.0, 8.6, 8.2, 7.8, 7.4, 7.0, 7.4, 7.8, 8.2, 8.6, 9.0, 21.0],
        [8.0, 7.6, 7.2, 6.8, 6.4, 6.0, 6.4, 6.8, 7.2, 7.6, 8.0, 21.0],
        [7.0, 6.6, 6.2, 5.8, 5.4, 5.0, 5.4, 5.8, 6.2, 6.6, 7.0, 21.0],
        [6.6, 5.6, 5.2, 4.8, 4.4, 4.0, 4.4, 4.8, 5.2, 5.6, 6.6, 21.0],
        [6.2, 5.2, 4.2, 3.8, 3.4, 3.0, 3.4, 3.8, 4.2, 5.2, 6.2, 21.0],
        [5.8, 4.8, 3.8, 2.8, 2.4, 2.0, 2.4, 2.8, 3.8, 4.8, 5.8, 21.0],
        [5.4, 4.4, 3.4, 2.4, 1.4, 1.0, 1.4, 2.4, 3.4, 4.4, 5.4, 21.0],
        [21.0, 21.0, 21.0, 21.0, 21.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]])
    assert np.abs(D - want).max() < 1e-5


def test_truncation_sees_the_float_sums():
    """Eight rows and five columns from a zero: five diagonal and three straight steps.  Added one at a time in float, most
    orders end at 10; three diagonal, three straight, two diagonal end just below it, and the minimum finds that chain -- so the
    window there is 9 wide at s = 10, not 10."""
    v = np.float32(0.0)
    for step in (1.4, 1.4, 1.4, 1.0, 1.0, 1.0, 1.4, 1.4):
        v = np.float32(v + np.float32(step))
    assert v < 10.0 and 10.0 - v < 2e-6 and int(v) == 9
    M = np.ones((40, 40), bool)
    M[20, 20] = False
    D = R.distance_map(M)
    assert D[28, 25] == v and D[12, 15] == v
    z = np.ones((40, 40), np.float32)
    rect = R.rect_map(z, D, 10.0)
    assert rect[28, 25] == 9 and rect[29, 29] == 10 and rect[22, 20] == 0 and rect[23, 20] == 3 and rect[9, 20] == 0
    assert R.rect_map(z, D, 3.5)[28, 25] == 3


def test_depth_change_map_by_hand():
    z = np.ones((5, 6), np.float32)
    z[2, 2] = 1.2                      # t = 0.02 * 2 * 2 = 0.08 at depth 1: a change to all four neighbours
    M = R.depth_change_map(z, 0.02)
    want = np.ones((5, 6), bool)
    want[2, 2] = want[2, 1] = want[2, 3] = want[1, 2] = want[3, 2] = False
    assert (M == want).all()
    z = np.ones((5, 6), np.float32)
    z[4, 2] = np.nan                   # the last row is nobody's centre: only the pixel above sees it
    z[1, 5] = 9.0                      # the last column likewise: only its left neighbour
    M = R.depth_change_map(z, 0.02)
    want = np.ones((5, 6), bool)
    want[4, 2] = want[3, 2] = want[1, 5] = want[1, 4] = False
    assert (M == want).all()


def test_python_surface_and_cpp_runner_compile(rs):
    from rsreg_amd import IntegralImageNormalEstimation, api, lib
    import ctypes as C
    assert IntegralImageNormalEstimation is api.IntegralImageNormalEstimation
    lib.build()
    p = api.iin_params()
    assert (p.method, p.depth_dependent_smoothing, p.border_policy, tuple(p.viewpoint)) == (1, 0, 0, (0.0, 0.0, 0.0))
    assert p.max_depth_change_factor == np.float32(0.02) and p.normal_smoothing_size == 10.0
    assert C.sizeof(lib.IinParams) == 32
    ne = IntegralImageNormalEstimation()
    ne.setNormalEstimationMethod(ne.AVERAGE_3D_GRADIENT)
    ne.setMaxDepthChangeFactor(0.02)
    ne.setNormalSmoothingSize(10.0)
    ne.setViewPoint(1, 2, 3)
    assert ne.getViewPoint() == (1.0, 2.0, 3.0) and ne.AVERAGE_3D_GRADIENT == lib.IIN_AVERAGE_3D_GRADIENT == 1
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "iinormals_runner.cpp")],
                   check=True)
