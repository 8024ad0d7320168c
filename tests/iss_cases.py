"""The inputs of tests/test_iss_cpu.py and tests/test_iss_gpu.py: the clouds of tests/radius_cases.py (imported, not copied), a case
worked out by hand, and the reference of every case computed once (tests/iss_ref.py) and left unchanged."""
import functools

import numpy as np

import iss_ref as I
import radius_cases as K
import radius_ref as R

# (cloud, salient radius, non-max radius)
CASES = [("uniform1000", 0.2, 0.12), ("uniform5000", 0.1, 0.06), ("sphere5000", 0.1, 0.06), ("non_finite", 0.15, 0.1),
         ("frame_pass", 0.06, 0.04), ("frame_pass", 0.03, 0.02), ("frame_raw", 0.06, 0.04),
         ("lattice", K.R_EDGE, K.R_FACE), ("lattice_pile", K.R_EDGE, K.R_FACE)]
CAPPED = [c for c in CASES if not c[0].startswith("lattice")]   # the lattices are all ties: exempt from the fragile-share cap
FRAGILE_CAP = 0.05                                              # the cap of tests/test_radius_gpu.py's normals

# The hand case: a record at (0, 0, 1) and six around it at +-2^-3 x, +-2^-4 y, +-2^-5 z -- every coordinate and difference exact.
# Radius 0.126 takes all six from the centre (2^-3 = 0.125 < 0.126): 7 neighbours, S = diag(2 * 2^-6, 2 * 2^-8, 2 * 2^-10) exactly,
# so the Jacobi has nothing to rotate: eigenvalues 2^-9, 2^-7, 2^-5, ratios 0.25 and 0.25, saliency 2^-9.  The six others have
# fewer: +-x see the centre alone (2), +-y and +-z see the centre and the four records on the other two short axes (5) -- the x
# records are sqrt(2^-6 + 2^-10) = 0.12885 from the z records, beyond 0.126.  (At 0.13, the radius first written down for this
# case, the z records reach the x records, have 7 neighbours and a larger saliency than the centre, 2^-7: the radius has to lie in
# (0.125, 0.12885].)
HAND_RADIUS, HAND_MIN_NEIGHBORS = 0.126, 7
HAND_EIG = (2.0 ** -9, 2.0 ** -7, 2.0 ** -5)


def hand_xyz():
    c = np.array([0.0, 0.0, 1.0])
    off = [(2.0 ** -3, 0, 0), (-2.0 ** -3, 0, 0), (0, 2.0 ** -4, 0), (0, -2.0 ** -4, 0), (0, 0, 2.0 ** -5), (0, 0, -2.0 ** -5)]
    return np.array([c] + [c + np.array(o) for o in off]).astype(np.float32)


def hand_cloud():
    return K.cloud(hand_xyz(), seed=11)


@functools.lru_cache(maxsize=None)
def search(name, radius):
    return R.search(K.input_cloud(name).xyz, radius)


@functools.lru_cache(maxsize=None)
def reference(name, salient, non_max, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    return I.detect(K.input_cloud(name).xyz, salient, non_max, gamma_21, gamma_32, min_neighbors, nb_s=search(name, salient), nb_n=search(name, non_max))


@functools.lru_cache(maxsize=None)
def fragile(name, salient, non_max):
    return I.fragile(reference(name, salient, non_max))


# ---- planted saliencies for rsreg_cloud_iss_non_max on the lattice (12^3, step H): INNER and its +x face neighbour
INNER = (5 * 12 + 5) * 12 + 5
FACE = INNER + 144                                             # (x is the slowest axis of radius_cases.lattice)


def planted(n, **at):
    """n zeros with the given values at the given records (keys: 'i<record>')."""
    s = np.zeros(n, np.float64)
    for k, v in at.items():
        s[int(k[1:])] = v
    return s
