"""Inputs of the FPFH tests (tests/test_fpfh_cpu.py, tests/test_fpfh_gpu.py): small clouds, float32 xyz, generated from fixed seeds."""
import functools

import numpy as np

H = 2.0 ** -6


def uniform(n=1500, seed=11):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * np.array([2.0, 1.5, 0.7]) + np.array([-1.0, -0.5, 0.4])).astype(np.float32)


def sphere(n=2000, seed=12):
    """A noisy shell of radius 0.5 in front of the viewpoint."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = 0.5 + 0.002 * rng.standard_normal(n)
    return (np.array([0.1, -0.2, 1.5]) + r[:, None] * u).astype(np.float32)


def corner(n=2000, seed=13):
    """A room corner: two noisy walls that meet at x = 0.5, y = 1.5."""
    rng = np.random.default_rng(seed)
    m = n // 2
    a = np.stack([rng.random(m) * 1.0 - 0.5, 1.5 + 0.002 * rng.standard_normal(m), rng.random(m) * 0.8 + 0.2], axis=1)
    b = np.stack([0.5 + 0.002 * rng.standard_normal(n - m), rng.random(n - m) * 1.0 + 0.5, rng.random(n - m) * 0.8 + 0.2], axis=1)
    return np.concatenate([a, b]).astype(np.float32)


def plane(m=30):
    """An m x m lattice with spacing 2^-6 in the plane z = 1: distance ties everywhere, every feature at mid-bin."""
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([g * H - 0.25, np.ones((len(g), 1))], axis=1).astype(np.float32)


def lattice(m=12):
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)
    return (g * H + np.array([0.0, 0.0, 1.0])).astype(np.float32)


def copies(seed=14):
    """The uniform box with exact copies: 12 copies of record 7 at the end (with k = 10 every one of them has only copies among
    its neighbours), and three copies of record 100 (a mixed neighbourhood for them and for the records around)."""
    xyz = uniform()
    return np.concatenate([xyz, np.repeat(xyz[7][None], 12, axis=0), np.repeat(xyz[100][None], 3, axis=0)]).astype(np.float32)


def holes(seed=15):
    """(xyz, the records whose NORMAL is to be made non-finite): the uniform box with 40 records of NaN / inf coordinates."""
    rng = np.random.default_rng(seed)
    xyz = uniform()
    bad = rng.choice(len(xyz), 40, replace=False)
    xyz[bad[:25]] = np.nan
    xyz[bad[25:], 1] = np.inf
    rest = np.setdiff1d(np.arange(len(xyz)), bad)
    return xyz, rng.choice(rest, 30, replace=False)


def many(n=66000, seed=16):
    """More records than the 65 536 workgroups of a launch."""
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * np.array([2.0, 1.5, 0.7]) + np.array([-1.0, -0.5, 0.4])).astype(np.float32)


def tiny(k, seed=17):
    """n = k records."""
    rng = np.random.default_rng(seed + k)
    return (rng.random((k, 3)) * 0.2 + np.array([0.0, 0.0, 1.0])).astype(np.float32)


CASES = {"uniform": uniform, "sphere": sphere, "corner": corner, "plane": plane, "lattice": lattice, "copies": copies}


@functools.lru_cache(maxsize=None)
def cloud(name):
    xyz = CASES[name]()
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def ref_normals(name, k=10):
    """The reference's normals (tests/normals_ref.py) of a case, float32 (n, 3): what the tests without a GPU feed the estimator."""
    import normals_ref as N
    nrm = np.ascontiguousarray(N.normals(cloud(name), k).normal)
    nrm.setflags(write=False)
    return nrm


# ---- hand-made normals: the contract normalises nothing, so its formulas hold for any finite normal.  Each case is (xyz, normals).
ZEROED = (200, 585)           # zero_normals: record 200 and its nearest neighbour, whose nearest neighbour is record 200
EVERY_K = tuple(range(2, 65))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def non_unit(power=0):
    """uniform() with its reference normals (k = 10), each times 2^e, e drawn from [-20, 20]: f2 and f3 leave [-1, 1] and the clamps
    of the bins at 0 and 10 work.  power: all of them times 2^power more (100: still finite floats, products far outside)."""
    e = np.random.default_rng(18).integers(-20, 21, len(cloud("uniform")))
    nrm = np.ldexp(ref_normals("uniform"), (e + power)[:, None]).astype(np.float32)
    assert np.isfinite(nrm).all()
    return _frozen(cloud("uniform").copy(), nrm)


@functools.lru_cache(maxsize=None)
def parallel():
    """lattice() with every normal (0, 0, 1): for the neighbours straight above and below dp is parallel to the source normal,
    |v| = 0, the pair is skipped.  Every other feature sits at mid-bin or well inside one."""
    xyz = lattice()
    return _frozen(xyz, np.tile(np.float32([0.0, 0.0, 1.0]), (len(xyz), 1)))


@functools.lru_cache(maxsize=None)
def zero_normals():
    """non_unit() with the normals of record ZEROED[0] and of its nearest neighbour set to (0, 0, 0): finite, so accepted.  One
    side zero: f1 = atan2(+-0, +-0), on the sign of a zero; both sides zero: v = 0, the pair is skipped both ways."""
    xyz, nrm = non_unit()
    nrm = nrm.copy()
    nrm[list(ZEROED)] = 0.0
    return _frozen(xyz.copy(), nrm)


@functools.lru_cache(maxsize=None)
def every_k():
    """200 records of the uniform box with their reference normals at k = 10: small enough to run every k from 2 to 64."""
    import normals_ref as N
    xyz = uniform(200, 3)
    return _frozen(xyz, np.ascontiguousarray(N.normals(xyz, 10).normal))


HAND_MADE = {"non_unit": non_unit, "non_unit_2^100": lambda: non_unit(100), "parallel": parallel, "zero_normals": zero_normals}
FRAGILE_CAP = {"non_unit": 0.01, "non_unit_2^100": 0.01, "parallel": 0.01, "zero_normals": 0.04}
