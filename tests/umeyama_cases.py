"""The case table of the Umeyama tests (tests/test_umeyama_cpu.py, tests/test_umeyama_gpu.py) and the drivers of their two
harnesses: tests/cpp/linalg_runner.cpp (g++, csrc/host_linalg.hpp on the host) and tests/cpp/solve.hip (hipcc, the two device
forms).  Every case is a pair of float32 clouds with a known motion and a fixed seed; the table is fixed, nothing is
filtered at run time."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import umeyama_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsense-pointcloud_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
RUNNER_SRC = os.path.join(ROOT, "tests", "cpp", "linalg_runner.cpp")
RUNNER = os.path.join(BUILD, "linalg_runner")
SOLVE_SRC = os.path.join(ROOT, "tests", "cpp", "solve.hip")
SOLVE_SO = os.path.join(BUILD, "solve.so")

SIZES = (3, 4, 7, 64, 1000)
f32 = np.float32
IDENT = np.eye(3).ravel()


# ------------------------------------------------------------------------------------------------ geometry
def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def move(P, R, t):
    """R p + t in f64 from the float32 points, rounded to float32 once."""
    return (P.astype(np.float64) @ np.asarray(R).T + np.asarray(t, np.float64)).astype(f32)


def sums_from_pairs(P, Q):
    """The 17 sums as the kernels' contract has them: f64, from the float32 values, added in index order."""
    p, q = P.astype(np.float64), Q.astype(np.float64)
    s = np.zeros(17)
    s[0] = len(p)
    if len(p):
        s[1:4] = np.cumsum(p, axis=0)[-1]
        s[4:7] = np.cumsum(q, axis=0)[-1]
        s[7:16] = np.cumsum((q[:, :, None] * p[:, None, :]).reshape(-1, 9), axis=0)[-1]   # (a product of two float32 is exact in f64)
        d = (Q - P).astype(f32)
        s[16] = np.cumsum((d.astype(np.float64) ** 2).sum(axis=1))[-1]
    return s


def sigma_as_the_code_does(sums):
    """sums / n - mu_q mu_p^T with one reciprocal, the operations and their order as in umeyama_from_sums (f64)."""
    inv_n = 1.0 / sums[0]
    mu_p, mu_q = sums[1:4] * inv_n, sums[4:7] * inv_n
    return (sums[7:16] * inv_n).reshape(3, 3) - mu_q[:, None] * mu_p[None, :]


# ------------------------------------------------------------------------------------------------ the table
def _case(cid, family, P, Q, posed="well", far=False, identity=False, exact_zero=False):
    P, Q = np.ascontiguousarray(P, f32), np.ascontiguousarray(Q, f32)
    assert P.shape == Q.shape and P.shape[1] == 3
    return {"id": cid, "family": family, "P": P, "Q": Q, "posed": posed, "far": far, "identity": identity, "exact_zero": exact_zero,
            "sums": sums_from_pairs(P, Q)}


def _table():
    cases = []
    tilt = rot([1.0, -2.0, 0.5], 25.0)

    for n in SIZES:   # full: a random cloud, a rotation of up to 30 degrees
        g = np.random.default_rng(1000 + n)
        P = (g.uniform(-1, 1, (n, 3)) + [0.3, -0.2, 1.5]).astype(f32)
        Q = move(P, rot(g.normal(size=3), g.uniform(5, 30)), g.uniform(-0.1, 0.1, 3))
        cases.append(_case("full-n%d" % n, "full", P, Q))

    for n in SIZES:   # wall: the plane z = 0, tilted; with and without 1 mm of noise on the target
        g = np.random.default_rng(2000 + n)
        flat = np.c_[g.uniform(-1, 1, (n, 2)), np.zeros(n)]
        P = (flat @ tilt.T + [0.1, 0.4, 2.0]).astype(f32)
        Q = move(P, rot(g.normal(size=3), g.uniform(2, 15)), g.uniform(-0.05, 0.05, 3))
        cases.append(_case("wall-n%d" % n, "wall", P, Q))
        cases.append(_case("wall-noise-n%d" % n, "wall", P, (Q + g.normal(0, 1e-3, (n, 3))).astype(f32)))

    for scale in (1e-3, 1e-6, 1e-9, 1e-12, 1e-14):   # thin: a slab, either side of the rank rule
        for n in SIZES:
            g = np.random.default_rng(3000 + n)
            slab = g.uniform(-1, 1, (n, 3)) * [1.0, 0.7, scale]
            # flat: the thin axis is z and the motion turns about z, so that the target is exactly as thin as the source
            P = slab.astype(f32)
            Q = move(P, rot([0, 0, 1], 12.0), [0.05, -0.02, 0.0])
            cases.append(_case("thin-flat-%g-n%d" % (scale, n), "thin", P, Q))
            # tilted: float32 rounding leaves a thickness of its own (some 1e-7 of the extent), with either sign of the determinant
            P = (slab @ tilt.T + [0.1, 0.4, 2.0]).astype(f32)
            Q = move(P, rot(g.normal(size=3), g.uniform(2, 15)), g.uniform(-0.05, 0.05, 3))
            cases.append(_case("thin-tilt-%g-n%d" % (scale, n), "thin", P, Q))

    for seed in (1, 2, 3):   # triangle: exactly three matches
        g = np.random.default_rng(4000 + seed)
        P = (g.uniform(-1, 1, (3, 3)) + [0.0, 0.0, 1.0]).astype(f32)
        Q = move(P, rot(g.normal(size=3), g.uniform(2, 25)), g.uniform(-0.1, 0.1, 3))
        cases.append(_case("triangle-%d" % seed, "triangle", P, Q))

    for n in SIZES:   # mirror: the target is the source seen in a mirror; axes scaled so that s2 and s3 are apart
        g = np.random.default_rng(5000 + n)
        P = (g.uniform(-1, 1, (n, 3)) * [1.0, 0.6, 0.3] + [0.2, 0.1, 1.0]).astype(f32)
        nrm = np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0])
        H = np.eye(3) - 2.0 * np.outer(nrm, nrm)
        cases.append(_case("mirror-n%d" % n, "mirror", P, move(P, rot([1, 1, 0], 7.0) @ H, [0.02, 0.0, -0.03])))

    for name, axis in (("x", [1, 0, 0]), ("y", [0, 1, 0]), ("z", [0, 0, 1]), ("skew", [0.3, -0.5, 0.8])):   # half-turn
        for deg in (179.0, 180.0):
            for n in SIZES:
                g = np.random.default_rng(6000 + n)
                P = (g.uniform(-1, 1, (n, 3)) * [1.0, 0.8, 0.6] + [0.1, -0.1, 0.5]).astype(f32)
                cases.append(_case("halfturn-%s-%g-n%d" % (name, deg, n), "half-turn", P, move(P, rot(axis, deg), [0.01, 0.02, -0.01])))

    for extent in (0.01, 0.1, 1.0):   # far: a small cloud a long way from the origin
        for n in SIZES:
            g = np.random.default_rng(7000 + n)
            P = (g.uniform(-0.5, 0.5, (n, 3)) * extent + [40.0, -30.0, 60.0]).astype(f32)
            c = P.astype(np.float64).mean(axis=0)
            R = rot(g.normal(size=3), 3.0)
            Q = move(P, R, c - R @ c + g.uniform(-0.1, 0.1, 3) * extent)   # (turned about its own centre)
            cases.append(_case("far-%g-n%d" % (extent, n), "far", P, Q, far=True))

    # equal-s: two or three equal singular values (the polar factor is unique, V is not)
    cube = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)])
    octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]) * 0.5
    for name, body in (("cube", cube), ("octahedron", octa), ("prism", cube * [1, 1, 0.5])):
        for k, R in enumerate((np.eye(3), rot([0.2, 0.9, -0.4], 20.0))):
            P = (body + [0.25, -0.5, 1.0]).astype(f32)
            cases.append(_case("equal-%s-%d" % (name, k), "equal-s", P, move(P, R, [0.125, 0.0, -0.0625])))

    # line: collinear, every coordinate dyadic so that the source is exactly on a line (ill-posed: the spin about it is free)
    for n in SIZES:
        g = np.random.default_rng(8000 + n)
        u = g.integers(-512, 512, n).astype(np.float64) / 1024.0
        u[:3] = [-0.5, 0.25, 0.5]
        P = (np.array([0.5, -0.25, 1.0]) + u[:, None] * np.array([1.0, 0.5, 0.25])).astype(f32)
        cases.append(_case("line-moved-n%d" % n, "line", P, move(P, rot([0.1, 1.0, 0.3], 9.0), [0.03, 0.01, -0.02]), posed="ill"))
        cases.append(_case("line-still-n%d" % n, "line", P, P.copy(), posed="ill", identity=True))

    # one-point: every source the same point, every target the same point; dyadic coordinates and a power of two of them, so
    # that sigma is exactly zero
    for n in (4, 64, 1024):
        for k, (p, q) in enumerate((([0.5, -0.25, 2.0], [0.75, 0.125, 1.5]), ([0.0, 0.0, 0.0], [0.0, 0.0, 0.0]))):
            cases.append(_case("onepoint-%d-n%d" % (k, n), "one-point", np.tile(p, (n, 1)), np.tile(q, (n, 1)), identity=True, exact_zero=True))

    for n in SIZES:   # near-one-point: the same with 1e-7 of float noise (ill-posed)
        g = np.random.default_rng(9000 + n)
        P = (np.tile([0.5, -0.25, 2.0], (n, 1)) + g.normal(0, 1e-7, (n, 3))).astype(f32)
        Q = (np.tile([0.75, 0.125, 1.5], (n, 1)) + g.normal(0, 1e-7, (n, 3))).astype(f32)
        cases.append(_case("near-onepoint-n%d" % n, "near-one-point", P, Q, posed="ill"))
    return cases


CASES = _table()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
FAMILIES = ("full", "wall", "thin", "triangle", "mirror", "half-turn", "far", "equal-s", "line", "one-point", "near-one-point")
assert {c["family"] for c in CASES} == set(FAMILIES)

# A matrix close to an orthogonal one far from the identity (row-major; orthonormalised() makes it one): the warm start of an
# alignment whose earlier iterations had nothing to do with the case at hand.
V_ARBITRARY = np.array([[-0.116, -0.520, -0.846], [-0.409, 0.801, -0.437], [0.905, 0.295, -0.306]])


def orthonormalised(V):
    u, _, vt = np.linalg.svd(V)
    return np.ascontiguousarray(u @ vt).ravel()


def slow_sequence(steps=10):
    """The sums of ten iterations of one alignment closing in: what the warm start was built for."""
    g = np.random.default_rng(77)
    P0 = (g.uniform(-1, 1, (500, 3)) + [0.0, 0.2, 1.5]).astype(f32)
    Q = move(P0, rot([0.3, 1.0, -0.2], 8.0), [0.05, -0.03, 0.02])
    out = []
    for k in range(steps):
        f = 0.6 ** k   # the source has covered 1 - f of the way
        P = move(P0, rot([0.3, 1.0, -0.2], 8.0 * (1 - f)), np.array([0.05, -0.03, 0.02]) * (1 - f))
        out.append((P, Q, sums_from_pairs(P, Q)))
    return out


U32 = 2.0 ** -23


def expected(case, ref):
    """(T_ref, bound): from the pairs; for the cases whose answer is the identity by rule, R = I and t = mu_q - mu_p."""
    if not case["identity"]:
        return ur.T_of(ref), ur.bound(ref, case["far"])
    pinned = dict(ref, R=np.eye(3), t=ref["mu_q"] - ref["mu_p"], s=np.array([1.0, 1.0, 0.0]), sign=1)
    return ur.T_of(pinned), ur.bound(pinned)


def check_rigid(T):
    """R R^T = I and det R = +1 to 4 float32 ulp (R's entries are float32: 3 products of rounded entries a dot product);
    the last row exactly (0, 0, 0, 1); everything finite."""
    T = np.asarray(T)
    assert T.dtype == np.float32 and np.isfinite(T).all()
    np.testing.assert_array_equal(T[3], np.array([0, 0, 0, 1], np.float32))
    R = T[:3, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 4 * U32, np.abs(R @ R.T - np.eye(3)).max()
    assert abs(np.linalg.det(R) - 1.0) <= 4 * U32, np.linalg.det(R)


SWEEP_DEGREES = (1.0, 3.0, 5.0, 7.0, 7.5, 8.0, 10.0, 15.0, 30.0, 45.0, 60.0, 89.0)


def completion_sweep(seeds=20):
    """Matrices of rank 1 and 2 with a V to start from, for jacobi_svd3: the column of V that completes U stands `deg`
    degrees off the columns of U already found, from well inside the switch to unit vectors (1/64 of its squared norm left:
    7.18 degrees) to square on.  Returns V0[n, 9], A[n, 9] and per row {"rank", "deg", "u", "v"}."""
    V0s, As, meta = [], [], []
    for seed in range(seeds):
        g = np.random.default_rng(500 + seed)
        V = np.linalg.qr(g.normal(size=(3, 3)))[0]
        v1, v2, v3 = V.T
        for deg in SWEEP_DEGREES:
            c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
            # rank 1: u1 stands deg off v2, the column that completes U next
            u1 = c * v2 + s * v1
            V0s.append(V.ravel()); As.append((0.7 * np.outer(u1, v1)).ravel()); meta.append({"rank": 1, "deg": deg})
            # rank 2: u1 = v1, u2 stands deg off v3
            u2 = c * v3 + s * v2
            V0s.append(V.ravel()); As.append((0.7 * np.outer(v1, v1) + 0.3 * np.outer(u2, v2)).ravel()); meta.append({"rank": 2, "deg": deg})
    return np.array(V0s), np.array(As), meta


# ------------------------------------------------------------------------------------------------ linalg_runner
def build_runner():
    os.makedirs(BUILD, exist_ok=True)
    tmp = "%s.%d.tmp" % (RUNNER, os.getpid())
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, RUNNER_SRC, "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout[-4000:]
    os.replace(tmp, RUNNER)
    return RUNNER


_OUT = {1: [("ok", "<i4", 1), ("T", "<f4", 16)], 2: [("ok", "<i4", 1), ("T", "<f4", 16), ("V", "<f8", 9)],
        3: [("U3", "<f8", 9), ("s3", "<f8", 3), ("V3", "<f8", 9), ("Ug", "<f8", 9), ("sg", "<f8", 3), ("Vg", "<f8", 9)],
        4: [("w", "<f8", 3), ("v", "<f8", 9)], 5: [("x", "<f8", 6)], 6: [("s", "<f8", 6)],
        7: [("U", "<f8", 9), ("s", "<f8", 3), ("V", "<f8", 9)]}


def run_runner(records, exe=None):
    """records: (op, payload...) -- (1, sums[n,17]), (2, v0[9], sums[n,17]), (3, A[n,9]), (4, A[n,9]), (5, A[n,36], b[n,6]),
    (6, A[n,36]), (7, V0[n,9], A[n,9]).  Returns, per record, a structured array with one row per case."""
    exe = exe or RUNNER
    blob, shapes = [], []
    for rec in records:
        op = rec[0]
        arrs = [np.ascontiguousarray(a, "<f8") for a in rec[1:]]
        n = arrs[-1].reshape(-1, {1: 17, 2: 17, 3: 9, 4: 9, 5: 6, 6: 36, 7: 9}[op]).shape[0]
        blob.append(np.array([op, n], "<i4").tobytes())
        if op in (5, 7):
            blob.append(np.concatenate([arrs[0].reshape(n, -1), arrs[1].reshape(n, -1)], axis=1).tobytes())
        else:
            blob.extend(a.tobytes() for a in arrs)
        shapes.append((op, n))
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "cases.bin"), os.path.join(d, "results.bin")
        with open(fin, "wb") as f:
            f.write(b"".join(blob))
        r = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0 and "%d records" % len(records) in r.stdout, r.stdout[-2000:]
        raw = open(fout, "rb").read()
    out, at = [], 0
    for op, n in shapes:
        dt = np.dtype([(name, t, (k,)) for name, t, k in _OUT[op]])
        out.append(np.frombuffer(raw, dt, n, at))
        at += dt.itemsize * n
    assert at == len(raw)
    return out


def T_rowmajor(t16):
    """The runner's and the library's column-major 16 floats as a 4 x 4."""
    return np.asarray(t16, f32).reshape(4, 4).T


# ------------------------------------------------------------------------------------------------ solve.hip
def build_solve():
    """tests/cpp/solve.hip -> tests/cpp/_build/solve.so with the library's own flags (gfx950, -O3, -ffp-contract=off)."""
    from rsreg_amd import lib

    os.makedirs(BUILD, exist_ok=True)
    tmp = "%s.%d.tmp" % (SOLVE_SO, os.getpid())
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *lib._flags(False), "-shared", "-I", lib.CSRC, "-I", os.path.join(ROOT, "include"),
           SOLVE_SRC, "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout[-4000:]
    os.replace(tmp, SOLVE_SO)
    return SOLVE_SO


def run_solve(sums, v_in, so=None):
    """One launch over all cases, a wave per case.  Returns {"T_lane", "V_lane", "ok_lane", "T_wave", "V_wave", "ok_wave"}."""
    h = ctypes.CDLL(so or SOLVE_SO)
    sums = np.ascontiguousarray(sums, np.float64).reshape(-1, 17)
    v_in = np.ascontiguousarray(v_in, np.float64).reshape(-1, 9)
    n = len(sums)
    assert len(v_in) == n
    out = {"T_lane": np.zeros((n, 16), f32), "V_lane": np.zeros((n, 9)), "ok_lane": np.zeros(n, np.int32),
           "T_wave": np.zeros((n, 16), f32), "V_wave": np.zeros((n, 9)), "ok_wave": np.zeros(n, np.int32)}
    vp = ctypes.c_void_p
    h.solve_cases.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    h.solve_cases.restype = ctypes.c_int
    rc = h.solve_cases(sums.ctypes.data, v_in.ctypes.data, n, *(out[k].ctypes.data for k in ("T_lane", "V_lane", "ok_lane", "T_wave", "V_wave", "ok_wave")))
    assert rc == 0, "solve_cases: hipError_t %d" % rc
    return out
