"""CPU: the reference of pcl::ISSKeypoint3D (tests/iss_ref.py) against a brute force and a case worked out by hand, the
condition of the GPU test's end-to-end check asserted on the reference alone, and the build: the library exports the entry
points, rsreg_iss_params has the size the header gives it, filters.hip compiles for gfx950 with both kernels free of spills and
scratch, and the adaptors refuse border estimation before any device call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import iss_cases as IC
import iss_ref as I
import radius_cases as K
import radius_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute(xyz, salient, non_max, gamma_21, gamma_32, min_neighbors):
    """An n x n float32 table and a loop per record: nothing shared with iss_ref but the formulas of include/rsreg.h."""
    from fitness_ref import d2_f32
    n = len(xyz)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = d2_f32(xyz[:, None, :], xyz[None, :, :])
    p = xyz.astype(np.float64)
    eig, sal = np.zeros((n, 3)), np.zeros(n)
    m_s = (d2 < R.r2_f32(salient)).sum(axis=1)
    for i in range(n):
        if m_s[i] < min_neighbors:
            continue
        d = p[d2[i] < R.r2_f32(salient)] - p[i]
        eig[i] = np.linalg.eigvalsh(d.T @ d)
        l3, l2, l1 = eig[i]
        if np.isfinite(eig[i]).all() and l3 >= 0 and l2 / l1 < gamma_21 and l3 / l2 < gamma_32:
            sal[i] = l3
    key = np.zeros(n, bool)
    for i in range(n):
        near = d2[i] < R.r2_f32(non_max)
        key[i] = sal[i] > 0 and near.sum() >= min_neighbors and not (sal[i] < sal[near]).any()
    return eig, sal, m_s, key


def test_reference_against_brute_force():
    xyz = K.uniform(1000, 1)
    r = I.detect(xyz, 0.2, 0.12)
    eig, sal, m_s, key = _brute(xyz, 0.2, 0.12, 0.975, 0.975, 5)
    np.testing.assert_array_equal(r.m_s, m_s)
    # the sums run in two orders (a matrix product here, reduceat there): m * 2^-53 of the moments, far below 1e-12 of the trace
    assert (np.abs(r.eig - eig) <= 1e-12 * r.trace[:, None]).all()
    assert ((r.saliency > 0) == (sal > 0)).all() and (np.abs(r.saliency - sal) <= 1e-12 * r.trace).all()
    np.testing.assert_array_equal(r.keypoint, key)
    assert 20 <= key.sum() <= 100                              # (46 when this was written)
    # the vectorised suppression against the loop on the SAME saliencies, NaN, negative, zero and +inf among them
    rng = np.random.default_rng(5)
    s = rng.random(1000)
    s[rng.integers(0, 1000, 60)] = np.nan
    s[rng.integers(0, 1000, 60)] = -1.0
    s[rng.integers(0, 1000, 60)] = 0.0
    s[rng.integers(0, 1000, 5)] = np.inf
    from fitness_ref import d2_f32
    d2 = d2_f32(xyz[:, None, :], xyz[None, :, :])
    for mn in (0, 5, 12):
        want = np.array([s[i] > 0 and (d2[i] < R.r2_f32(0.12)).sum() >= mn and not (s[i] < s[d2[i] < R.r2_f32(0.12)]).any() for i in range(1000)])
        np.testing.assert_array_equal(I.non_max(s, r.nb_n, mn), want)


def test_hand_case():
    xyz = IC.hand_xyz()
    r = I.detect(xyz, IC.HAND_RADIUS, IC.HAND_RADIUS, min_neighbors=IC.HAND_MIN_NEIGHBORS)
    assert r.m_s.tolist() == [7, 2, 2, 5, 5, 5, 5]
    assert tuple(r.S[0].diagonal()) == (2.0 ** -5, 2.0 ** -7, 2.0 ** -9) and (r.S[0] == np.diag(r.S[0].diagonal())).all()
    assert tuple(r.eig[0]) == IC.HAND_EIG and (r.eig[1:] == 0).all()
    assert r.saliency.tolist() == [2.0 ** -9] + [0.0] * 6 and r.indices.tolist() == [0]
    at = I.detect(xyz, IC.HAND_RADIUS, IC.HAND_RADIUS, gamma_21=0.25, min_neighbors=IC.HAND_MIN_NEIGHBORS)      # 0.25 < 0.25 fails
    assert (at.saliency == 0).all() and len(at.indices) == 0
    above = I.detect(xyz, IC.HAND_RADIUS, IC.HAND_RADIUS, gamma_21=float(np.nextafter(0.25, 1)), min_neighbors=IC.HAND_MIN_NEIGHBORS)
    assert above.indices.tolist() == [0]
    assert len(I.detect(xyz, IC.HAND_RADIUS, IC.HAND_RADIUS, gamma_32=0.25, min_neighbors=IC.HAND_MIN_NEIGHBORS).indices) == 0
    assert len(I.detect(xyz, IC.HAND_RADIUS, IC.HAND_RADIUS, min_neighbors=8).indices) == 0


def test_lattice_is_exact_and_all_ties():
    """Every sum of the lattice is exact: an inner record's scatter over its 1 + 6 + 12 neighbours is 10 H^2 I, its saliency the
    same number as every other inner record's, and the strict compare keeps them all."""
    r = IC.reference("lattice", K.R_EDGE, K.R_FACE)
    assert (r.S[IC.INNER] == np.eye(3) * 10 * K.H ** 2).all() and r.m_s[IC.INNER] == 19
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 3)
    inside = ((g > 0) & (g < 11)).all(axis=1)
    assert (r.trace[inside] == 30 * K.H ** 2).all()
    # three equal eigenvalues: the ratios are 1, not below 0.975 -- no inner record is salient; with gammas above 1 they all are
    assert (r.saliency[inside] == 0).all()
    loose = I.detect(K.lattice(12), K.R_EDGE, K.R_FACE, 1.5, 1.5, 5, nb_s=r.nb_s, nb_n=r.nb_n)
    assert (np.abs(loose.saliency[inside] - 10 * K.H ** 2) <= 1e-12 * 30 * K.H ** 2).all()


@pytest.mark.parametrize("name,salient,non_max", IC.CAPPED)
def test_fragile_share_is_capped(name, salient, non_max):
    """The condition of tests/test_iss_gpu.py's end-to-end check, on the reference alone: at most 5 % of the finite records are
    fragile (iss_ref.fragile).  Measured when this was written: 0 on the synthetic clouds, 0.14 % / 1.6 % / 0.12 % on the frames."""
    r = IC.reference(name, salient, non_max)
    f = IC.fragile(name, salient, non_max)
    fin = r.nb_s.fin
    share = f[fin].mean()
    print("iss fragile share: %s %g / %g: %d keypoints, m_s %d .. %d, fragile %d of %d = %.3f %%" %
          (name, salient, non_max, len(r.indices), r.m_s[fin].min(), r.m_s[fin].max(), int(f.sum()), int(fin.sum()), 100 * share))
    assert not f[~fin].any() and share <= IC.FRAGILE_CAP
    assert len(r.indices) > 0 and (np.diff(r.indices) > 0).all()


def test_library_and_adaptors(rs):
    from rsreg_amd import ISSKeypoint3D, api, lib
    lib.build()
    handle = lib.lib()
    for name in ("rsreg_iss_params_default", "rsreg_cloud_iss_saliency", "rsreg_cloud_iss_non_max", "rsreg_cloud_iss_keypoints"):
        assert name in lib.EXPORTS and getattr(handle, name) is not None
    assert "iss_kernels.hpp" in lib.HEADERS and "filters.hip" in lib.SOURCES and not any("iss" in s for s in lib.SOURCES)
    assert ctypes.sizeof(lib.IssParams) == 40
    p = api.iss_params()
    assert (p.salient_radius, p.non_max_radius, p.gamma_21, p.gamma_32, p.min_neighbors, p.reserved) == (0.0, 0.0, 0.975, 0.975, 5, 0)
    assert api.iss_params(salient_radius=0.06, min_neighbors=7).min_neighbors == 7
    with pytest.raises(lib.RsregError):
        api.iss_params(salient=0.06)
    assert ISSKeypoint3D is api.ISSKeypoint3D
    for name in ("iss_keypoints", "iss_saliency", "iss_non_max"):
        assert hasattr(api.DeviceCloud, name)
    iss = ISSKeypoint3D()
    assert (iss.salient_radius, iss.non_max_radius, iss.gamma_21, iss.gamma_32, iss.min_neighbors) == (0.0, 0.0, 0.975, 0.975, 5)   # PCL's defaults
    iss.setInputCloud(IC.hand_cloud())
    iss.setSalientRadius(0.126)
    iss.setNonMaxRadius(0.1)
    iss.setThreshold21(0.5)
    iss.setThreshold32(0.6)
    iss.setMinNeighbors(7)
    assert (iss.salient_radius, iss.non_max_radius, iss.gamma_21, iss.gamma_32, iss.min_neighbors) == (0.126, 0.1, 0.5, 0.6, 7)
    for setter in (iss.setBorderRadius, iss.setNormalRadius):  # not built: refused before any device call -- there is no device here
        setter(0.1)
        with pytest.raises(lib.RsregError, match="not built") as e:
            iss.compute()
        assert e.value.status == lib.RSREG_ERR_INVALID_ARG
        setter(0.0)
    assert len(iss.getKeypointsIndices()) == 0


def test_filters_compile_for_gfx950_without_spill_or_scratch(tmp_path):
    """hipcc cross-compiles filters.hip (which includes iss_kernels.hpp) for gfx950; the compiler's resource remarks show neither
    new kernel spilling or using scratch, and no LDS."""
    from rsreg_amd import lib
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, *lib._flags(False), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(lib.CSRC, "filters.hip"), "-o", str(tmp_path / "filters.dev.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    blocks = re.split(r"remark: Function Name: ", r.stdout)
    for kernel in ("k_iss_saliency", "k_iss_non_max"):
        mine = [b for b in blocks if re.match(r"_ZN5rsreg\d+%sE" % kernel, b)]
        assert len(mine) == 1, kernel
        fig = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\d+)", mine[0])}
        print(kernel, fig)
        assert fig["ScratchSize [bytes/lane]"] == 0 and fig["SGPRs Spill"] == 0 and fig["VGPRs Spill"] == 0 and fig["LDS Size [bytes/block]"] == 0


def test_cpp_adaptor_refuses_border_estimation(rs):
    """tests/cpp/iss_runner.cpp compiles with a host compiler, and its `refuse` mode sees rsreg::ISSKeypoint3D throw
    RSREG_ERR_INVALID_ARG for setBorderRadius(0.1) and for setNormalRadius(0.1) without a device."""
    from rsreg_amd import lib
    lib.build()
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "iss_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "iss_runner.cpp"),
                        "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe, "refuse"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "refused yes", r.stdout
