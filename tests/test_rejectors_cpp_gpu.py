"""The C++ adaptor of the rejector chain (include/rsreg/pcl_compat.hpp: rsreg::registration::CorrespondenceRejector*,
addCorrespondenceRejector and its companions) compiles and gives the Python layer's answer -- which tests/test_rejectors_gpu.py
holds to the reference -- bit for bit: the final 4 x 4, the pair count and every rejector's counts and median
(tests/cpp/rejector_runner.cpp)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_cpp_adaptor_gives_the_python_layers_chain(tmp_path):
    from rsreg_amd import api, synth
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "rejector_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "rejector_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    tgt = synth.render_frame(0, (160, 120), "bench")
    src = synth.render_frame(1, (160, 120), "bench")
    k, iterations = 10, 6
    ctx = api.Context(0)
    nrm = {}
    for name, cloud in (("src", src), ("tgt", tgt)):
        dev = api.DeviceCloud(cloud, ctx=ctx)
        dn = dev.normals_cloud(k)
        nrm[name] = dn.download_normals()
        dn.close()
        dev.close()

    def records48(cloud, normals):
        rec = np.zeros(len(cloud.points), api.POINT_NORMAL_DTYPE)
        for f in ("x", "y", "z", "rgba"):
            rec[f] = cloud.points[f]
        rec["w"] = 1.0
        for f in ("normal_x", "normal_y", "normal_z", "curvature"):
            rec[f] = normals.points[f]
        return rec

    def run(cls, source, target, rejectors, src_n=None, tgt_n=None):
        icp = cls(ctx)
        icp.setMaxCorrespondenceDistance(0.05)
        icp.setMaximumIterations(iterations)
        icp.setCriteriaMode(1)
        for r in rejectors:
            icp.addCorrespondenceRejector(r)
        icp.setInputSource(source)
        icp.setInputTarget(target)
        if src_n is not None:
            icp.setInputSourceNormals(src_n)
            icp.setInputTargetNormals(tgt_n)
        icp.align()
        return icp, (icp.rejector_stats() if rejectors else [])

    M, O, S, T = (api.CorrespondenceRejectorMedianDistance, api.CorrespondenceRejectorOneToOne, api.CorrespondenceRejectorSurfaceNormal,
                  api.CorrespondenceRejectorTrimmed)
    want = {
        "points": run(api.IterativeClosestPoint, src, tgt, [O(), M()]),
        "plain": run(api.IterativeClosestPoint, src, tgt, []),
        "normals": run(api.IterativeClosestPoint, records48(src, nrm["src"]), records48(tgt, nrm["tgt"]), [S(0.7), M(1.5)]),
        "beside": run(api.IterativeClosestPointWithNormals, src, tgt, [S(0.7), T(0.8)], nrm["src"], nrm["tgt"]),
    }
    assert want["points"][0].result.n_correspondences < want["plain"][0].result.n_correspondences      # the chain does remove pairs
    assert bytes(want["points"][0].result.transform) != bytes(want["plain"][0].result.transform)
    assert want["normals"][1][0][1] < want["normals"][1][0][0] and want["beside"][1][0][1] < want["beside"][1][0][0]

    src.points.tofile(str(tmp_path / "src.bin"))
    tgt.points.tofile(str(tmp_path / "tgt.bin"))
    nrm["src"].points.tofile(str(tmp_path / "src_n.bin"))
    nrm["tgt"].points.tofile(str(tmp_path / "tgt_n.bin"))
    r = subprocess.run([exe, str(tmp_path / "src.bin"), str(len(src)), str(tmp_path / "tgt.bin"), str(len(tgt)), str(tmp_path / "src_n.bin"),
                        str(tmp_path / "tgt_n.bin"), str(iterations)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    lines = {l.split()[0]: l for l in r.stdout.strip().splitlines()}
    for route, (icp, stats) in want.items():
        head, *per = lines[route].split(" | ")
        f = head.split()[1:]
        words = np.array([int(w, 16) for w in f[:16]], np.uint32)
        assert words.tobytes() == bytes(icp.result.transform), (route, r.stdout)
        assert int(f[17]) == iterations and int(f[19]) == icp.result.n_correspondences
        got = [(int(p.split()[0]), int(p.split()[1]), float(p.split()[2])) for p in per]
        assert got == stats, (route, got, stats)
    assert float(lines["median"].split()[1]) == want["points"][1][1][2] > 0
