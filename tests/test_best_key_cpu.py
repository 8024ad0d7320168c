"""csrc/icp_dense.hpp keeps the running best of a search as the key d_bits << 32 | index read as an IEEE double and takes minima
with the f64 minimum instruction.  That is the unsigned 64-bit minimum as long as every key is a finite non-negative double --
which d >= 0 (bits 0 ... 0x7f800000) makes it.  Checked on the host with fmin (CPU only, g++) at the edge patterns: d bits 0, 1,
0x007fffff (the key is then a subnormal double), 0x7f7fffff, 0x7f800000; index 0, 1, 0xfffffffe, 0xffffffff; equal d."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "best_key.cpp")


def test_f64_minimum_of_keys_is_the_u64_minimum():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "best_key")
        r = subprocess.run(["g++", "-std=c++17", "-O1", SRC, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    m = re.search(r"best_key ok: (\d+) pairs", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) >= 7 * 4 * 7 * 4, r.stdout[-3000:]
