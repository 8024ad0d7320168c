"""csrc/ring1_offsets.hpp says where neighbour j of a cell lies in the padded table and which gap a search step picks per
axis; the GPU search fills its 27-word table with that function (icp_dense.hpp: dense_ring1_setup).  Checked on the host
against the plain formula (dz - 1) * sxy + (dy - 1) * sx + (dx - 1) for all 27 j over edge dimensions 1, 2, 4 000 and
strides up to sx * sy = 2^28 (CPU only, g++, a stand-alone program under the address and undefined-behaviour sanitizers)."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ring1_offsets.cpp")
INC = os.path.join(ROOT, "realsense-pointcloud_amd", "csrc")


def test_ring1_offsets_match_the_plain_formula():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ring1_offsets")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    m = re.search(r"ring1_offsets ok: (\d+) checks", r.stdout)
    # 6 x 6 grids less the ones beyond 2^28 (at least 30), 27 neighbours, three checks each
    assert r.returncode == 0 and m and int(m.group(1)) >= 30 * 27 * 3, r.stdout[-3000:]
