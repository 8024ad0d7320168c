"""The host side of the tile schedule (csrc/tile_sched.hpp), checked on the CPU: which launch of an alignment is plain, timed,
served by the kept first-launch schedule or by the steady one, when a kept schedule expires or no longer fits, and where the
arrays lie in the schedule buffer.  tests/cpp/tile_sched_rule.cpp includes that header alone, is compiled with plain g++ -- no
HIP, no GPU -- and run under AddressSanitizer and UBSan."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tile_sched_rule.cpp")


def test_tile_schedule_rule_under_sanitizer():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "tile_sched_rule")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
        assert r.returncode == 0 and "tile schedule rule ok" in r.stdout, r.stdout[-4000:]
