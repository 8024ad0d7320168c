"""The C++ adaptor of GICP (include/rsreg/pcl_compat.hpp: GeneralizedIterativeClosestPoint) gives the 4 x 4, the counts and the
fitness score of the Python layer, bit for bit: with the covariances handed in, and with none given, when the class computes
them itself on a device cloud as PCL does (tests/cpp/gicp_runner.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import gicp_cases as GC
import plane_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_cpp_adaptor_gives_the_python_layers_transform(tmp_path):
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "gicp_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gicp_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    c = GC.align_case("walls5k")
    gate, eps, k = c.prm.max_correspondence_distance, 1e-7, GC.K
    src, tgt = PC.cloud(c.src), PC.cloud(c.tgt)
    ctx = api.Context(0)

    def run(cov_s, cov_t):
        g = GC.make_gicp(api, ctx, src, tgt, cov_s, cov_t, gate, **GC.TIGHT)
        g.setCorrespondenceRandomness(k)
        g.align()
        g.fitness = g.getFitnessScore(0.0025)   # (of this object's alignment: the context is the next object's afterwards)
        return g

    given, computed = run(c.cov_s, c.cov_t), run(None, None)
    assert given.hasConverged() and computed.hasConverged() and given.result.n_correspondences == 5000
    src.points.tofile(str(tmp_path / "src.bin"))
    tgt.points.tofile(str(tmp_path / "tgt.bin"))
    np.ascontiguousarray(c.cov_s).tofile(str(tmp_path / "cs.bin"))
    np.ascontiguousarray(c.cov_t).tofile(str(tmp_path / "ct.bin"))
    r = subprocess.run([exe, str(tmp_path / "src.bin"), str(len(src)), str(tmp_path / "tgt.bin"), str(len(tgt)), str(tmp_path / "cs.bin"),
                        str(tmp_path / "ct.bin"), repr(gate), repr(eps), str(k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    lines = {l.split()[0]: l.split()[1:] for l in r.stdout.strip().splitlines()}
    for route, g in (("given", given), ("computed", computed)):
        words = np.array([int(w, 16) for w in lines[route][:16]], np.uint32)
        assert words.tobytes() == bytes(g.result.transform), (route, r.stdout)
        assert int(lines[route][17]) == g.result.iterations and int(lines[route][19]) == g.result.inner_evaluations
        assert int(lines[route][21]) == g.result.n_correspondences and int(lines[route][23]) == 1
        assert float(lines[route][25]) == g.fitness
