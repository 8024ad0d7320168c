"""GPU: rsreg::VoxelGrid of include/rsreg/pcl_compat.hpp (tests/cpp/voxelgrid_runner.cpp) on host and device clouds gives the
bytes the numpy reference gives, and PCL's getters what the reference's info holds."""
import os
import subprocess

import numpy as np
import pytest

import voxelgrid_cases as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(rs):
    from rsreg_amd import api, lib
    lib.build()
    if api.device_count() < 1:
        pytest.fail("no HIP device: the product has no CPU fallback")
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "voxelgrid_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "voxelgrid_runner.cpp"),
                    "-o", path, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    return path


@pytest.mark.parametrize("name", ["run_classes_min2", "non_finite_in_dense_cloud", "boundaries_aniso"])
def test_cpp_adaptor(exe, tmp_path, name):
    pts, leaf, _, mp = V.cases()[name]
    want, info = V.reference(name)
    np.ascontiguousarray(pts).tofile(str(tmp_path / "in.bin"))
    outs = [str(tmp_path / f) for f in ("host.bin", "gpu.bin", "dev.bin")]
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(len(pts)), *[repr(float(np.float32(v))) for v in leaf], str(mp), *outs],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    vals = dict(l.split() for l in r.stdout.strip().splitlines())
    for path in outs:
        got = np.fromfile(path, dtype=np.uint8)
        np.testing.assert_array_equal(got, want.view(np.uint8).reshape(-1))
    assert int(vals["host"]) == int(vals["gpu"]) == int(vals["device"]) == int(vals["width"]) == len(want)
    assert (vals["height"], vals["dense"]) == ("1", "1") and int(vals["leaves"]) == info["n_leaves"]
    for key in ("div_b", "min_b", "max_b", "divb_mul"):
        assert [int(v) for v in vals[key].split(",")] == info[key]
