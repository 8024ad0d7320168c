"""GPU: rsreg::DepthToCloud of include/rsreg/capture.hpp (tests/cpp/depthcloud_runner.cpp) into a host cloud and into a device
cloud gives the bytes the C ABI gives, which are the numpy reference's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depthcase_cases as D

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
    path = os.path.join(out, "depthcloud_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "depthcloud_runner.cpp"),
                    "-o", path, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    return path


@pytest.mark.parametrize("name,crop", [("distortion_both", 0), ("reference_13x7", 1), ("padded_bpp4_rgb", 0)])
def test_cpp_class(rs, exe, tmp_path, name, crop):
    from rsreg_amd import lib
    case = D.cases()[name]
    want, meta, _ = D.reference(name)
    q = D.c_params(lib, case.p)
    (tmp_path / "params.bin").write_bytes(bytes(memoryview(q)))
    case.dbuf.tofile(str(tmp_path / "depth.bin"))
    case.cbuf.tofile(str(tmp_path / "color.bin"))
    outs = [str(tmp_path / f) for f in ("host.bin", "device.bin", "abi.bin")]
    r = subprocess.run([exe, str(tmp_path / "params.bin"), str(tmp_path / "depth.bin"), str(case.dstride), str(tmp_path / "color.bin"), str(case.cstride),
                        str(crop), *outs], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    abi = np.fromfile(outs[2], dtype=np.uint8)
    for path in outs:
        got = np.fromfile(path, dtype=np.uint8)
        np.testing.assert_array_equal(got, abi)
        np.testing.assert_array_equal(got, want.view(np.uint8).reshape(-1))
    vals = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in r.stdout.strip().splitlines()}
    assert vals["host"] == vals["device"] == vals["abi"] == [meta[0], meta[2], meta[3], meta[4]]
