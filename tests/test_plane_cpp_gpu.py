"""The C++ adaptor of point-to-plane ICP (include/rsreg/pcl_compat.hpp: PointXYZRGBNormal, IterativeClosestPointWithNormals)
gives the 4 x 4 of the Python layer, bit for bit: on host clouds of 48-byte records that carry their normals, and on device
clouds through NormalEstimation -> setInputTargetNormals (tests/cpp/plane_runner.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import plane_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_cpp_adaptor_gives_the_python_layers_transform(tmp_path):
    from rsreg_amd import api, synth
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "plane_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "plane_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    tgt = synth.render_frame(0, (160, 120), "bench")
    src = synth.render_frame(1, (160, 120), "bench")
    k, iterations = 10, 6
    ctx = api.Context(0)
    dev_tgt = api.DeviceCloud(tgt, ctx=ctx)
    dev_nrm = dev_tgt.normals_cloud(k)
    nrm = dev_nrm.download_normals()

    def records48(cloud, normals=None):
        rec = np.zeros(len(cloud.points), api.POINT_NORMAL_DTYPE)
        for f in ("x", "y", "z", "rgba"):
            rec[f] = cloud.points[f]
        rec["w"] = 1.0
        if normals is not None:
            for f in ("normal_x", "normal_y", "normal_z", "curvature"):
                rec[f] = normals.points[f]
        return rec

    def run(source, target, normals):
        icp = api.IterativeClosestPointWithNormals(ctx)
        icp.setMaxCorrespondenceDistance(PC.GATE)
        icp.setMaximumIterations(iterations)
        icp.setCriteriaMode(1)
        icp.setInputSource(source)
        icp.setInputTarget(target, normals)
        icp.align()
        return icp

    by_records = run(records48(src), records48(tgt, nrm), None)
    by_device = run(api.DeviceCloud(src, ctx=ctx), dev_tgt, dev_nrm)
    assert by_records.result.iterations == iterations and by_records.result.n_correspondences > 5000
    assert bytes(by_records.result.transform) == bytes(by_device.result.transform)

    src.points.tofile(str(tmp_path / "src.bin"))
    tgt.points.tofile(str(tmp_path / "tgt.bin"))
    nrm.points.tofile(str(tmp_path / "nrm.bin"))
    r = subprocess.run([exe, str(tmp_path / "src.bin"), str(len(src)), str(tmp_path / "tgt.bin"), str(len(tgt)), str(tmp_path / "nrm.bin"),
                        str(k), str(iterations)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    lines = {l.split()[0]: l.split()[1:] for l in r.stdout.strip().splitlines()}
    for route, icp in (("records", by_records), ("device", by_device)):
        words = np.array([int(w, 16) for w in lines[route][:16]], np.uint32)
        assert words.tobytes() == bytes(icp.result.transform), (route, r.stdout)
        assert int(lines[route][17]) == iterations and int(lines[route][19]) == icp.result.n_correspondences
    assert float(lines["fitness"][0]) == by_device.getFitnessScore(0.0025)
