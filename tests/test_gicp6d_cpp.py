"""The C++ adaptor of GICP6D (include/rsreg/pcl_compat.hpp: GeneralizedIterativeClosestPoint6D) gives the 4 x 4 and the counts of the
Python layer on the scene of tests/gicp6d_cases.py, bit for bit: with the colours handed in, and with none given, when the class
converts the clouds' own rgb words (tests/cpp/gicp6d_runner.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import gicp6d_cases as GC6
import gicp_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_cpp_adaptor_gives_the_python_layers_transform(tmp_path):
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "gicp6d_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gicp6d_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    c = GC6.scene()
    src, tgt = GC6.rgb_cloud(c.src, c.rgba_s), GC6.rgb_cloud(c.tgt, c.rgba_t)
    lab_s, lab_t = api.rgb_to_lab(c.rgba_s), api.rgb_to_lab(c.rgba_t)
    ctx = api.Context(0)

    def run(ls, lt):
        g = api.GeneralizedIterativeClosestPoint6D(ctx, lab_weight=GC6.SCENE_WEIGHT)
        g.setMaxCorrespondenceDistance(GC6.SCENE_GATE)
        for k, v in GC.TIGHT.items():
            setattr(g.gparams, k, v)
        g.setInputSource(src)
        g.setInputTarget(tgt)
        g.setSourceCovariances(c.cov_s)
        g.setTargetCovariances(c.cov_t)
        if ls is not None:
            g.setSourceLab(ls)
            g.setTargetLab(lt)
        g.align()
        return g

    given, computed = run(lab_s, lab_t), run(None, None)
    assert given.hasConverged() and given.result.n_correspondences == len(c.src)
    assert bytes(given.result.transform) == bytes(computed.result.transform)
    assert float(np.linalg.norm(given.getFinalTransformation().astype(np.float64) - c.truth)) < 1e-3
    files = {}
    for name, a in (("src", src.points), ("tgt", tgt.points), ("cs", c.cov_s), ("ct", c.cov_t), ("ls", lab_s), ("lt", lab_t)):
        files[name] = str(tmp_path / (name + ".bin"))
        np.ascontiguousarray(a).tofile(files[name])
    r = subprocess.run([exe, files["src"], str(len(src)), files["tgt"], str(len(tgt)), files["cs"], files["ct"], files["ls"], files["lt"],
                        repr(GC6.SCENE_GATE), repr(GC.TIGHT["transformation_epsilon"]), repr(GC6.SCENE_WEIGHT)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    lines = {l.split()[0]: l.split()[1:] for l in r.stdout.strip().splitlines()}
    for route, g in (("given", given), ("computed", computed)):
        words = np.array([int(w, 16) for w in lines[route][:16]], np.uint32)
        assert words.tobytes() == bytes(g.result.transform), (route, r.stdout)
        assert int(lines[route][17]) == g.result.iterations and int(lines[route][19]) == g.result.inner_evaluations
        assert int(lines[route][21]) == g.result.n_correspondences and int(lines[route][23]) == 1
