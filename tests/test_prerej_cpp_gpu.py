"""tests/cpp/prerej_runner.cpp (rsreg::SampleConsensusPrerejective of include/rsreg/pcl_compat.hpp) on a constructed pair: the C++
class gives the transform, the inliers and the aligned cloud of the Python calls, from host clouds and from clouds that stay in HBM."""
import os
import subprocess

import numpy as np
import pytest

import prerej_cases as C
import prerej_ref as R
import sac_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_cpp_class_gives_the_python_paths_bytes(tmp_path):
    from rsreg_amd import api
    if api.device_count() < 1:
        pytest.fail("no HIP device")
    ctx = api.Context(0)
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "prerej_runner")
    pkg = os.path.join(ROOT, "realsense-pointcloud_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "prerej_runner.cpp"),
                    "-o", exe, "-L", pkg, "-lrsreg", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    # 400 points and their copy moved by 120 degrees and 0.5 m; 60 % of the source's descriptors are their target record's, the rest
    # are random: the table rsreg_cloud_feature_knn makes of them holds the true match first in those rows
    src, tgt, true_of = C.pair(400, 12)
    rng = np.random.default_rng(6)
    ftgt = rng.random((400, 33)).astype(np.float32)
    fsrc = ftgt[true_of].copy()
    lost = rng.random(400) < 0.4
    fsrc[lost] = rng.random((int(lost.sum()), 33)).astype(np.float32)
    rec = lambda f: np.ascontiguousarray(f).view(api.FPFH_DTYPE).reshape(-1)
    K.records(src, 32).tofile(str(tmp_path / "source.bin"))
    K.records(tgt, 32, 1).tofile(str(tmp_path / "target.bin"))
    rec(fsrc).tofile(str(tmp_path / "sfeat.bin"))
    rec(ftgt).tofile(str(tmp_path / "tfeat.bin"))
    dev = lambda xyz, seed: api.DeviceCloud(api.NormalCloud(K.records(xyz, 32, seed), len(xyz), 1, False), ctx=ctx)
    dsrc, dtgt = dev(src, 0), dev(tgt, 1)
    dfs, dft = (api.DeviceCloud(api.FPFHCloud(rec(f), len(f), 1, True), ctx=ctx) for f in (fsrc, ftgt))
    for by_inliers in (0, 1):
        prefix = str(tmp_path / ("run%d_" % by_inliers))
        r = subprocess.run([exe, str(tmp_path / "source.bin"), str(tmp_path / "target.bin"), str(tmp_path / "sfeat.bin"), str(tmp_path / "tfeat.bin"),
                            "0.05", "256", "21", "2", str(by_inliers), prefix], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout
        vals = dict(l.split() for l in r.stdout.strip().splitlines())
        nbr, _ = dfs.feature_knn(dft, 2)
        assert (nbr[~lost, 0] == true_of[~lost]).all()
        prm = dict(max_iterations=256, similarity_threshold=0.9, max_correspondence_distance=0.05, inlier_fraction=0.25, seed=21, select_by_inliers=by_inliers)
        inliers, res = dsrc.prerejective(dtgt, nbr, **prm)
        want = R.prerejective(api, src, tgt, nbr, **prm)
        assert res.found and res.n_inliers == 400 and want.best_hypothesis == res.best_hypothesis
        assert res.transform.tobytes() == np.asarray(want.transform, np.float32).tobytes()
        moved = api.transformPointCloud(dsrc, res.transform)
        moved_bytes = np.zeros(400 * 32, np.uint8)
        from rsreg_amd import lib as L
        L.check(L.lib().rsreg_cloud_download(moved.h, moved_bytes.ctypes.data, 400), ctx.h)
        assert vals["refused_4_samples"] == "1"
        for side in ("host", "device"):
            assert vals["converged_" + side] == "1" and int(vals["inliers_" + side]) == 400 and float(vals["fitness_" + side]) == res.fitness
            assert open(prefix + "inliers_%s.bin" % side, "rb").read() == inliers.tobytes()
            assert open(prefix + "t_%s.bin" % side, "rb").read() == np.ascontiguousarray(res.transform.T).tobytes()
            aligned = np.fromfile(prefix + "aligned_%s.bin" % side, np.float32).reshape(400, 8)[:, :3]
            assert aligned.tobytes() == np.ascontiguousarray(moved_bytes.view(np.float32).reshape(400, 8)[:, :3]).tobytes(), side
    ctx.close()
