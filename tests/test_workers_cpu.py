"""The context's helper threads (csrc/workers.hpp) under ThreadSanitizer and AddressSanitizer, with stub jobs (CPU only).

They carry the source load beside the index build (incremental_icp.hpp:57-58: setInputSource, setInputTarget), the frame
uploads / side jobs of the scheme loops (types.hpp:30-43) and the streamed download of the merged cloud."""
import os
import platform
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "workers_tsan.cpp")


def _no_aslr():
    """`setarch <arch> -R`: this one process without address randomisation, where the host allows it.  GCC 11's
    ThreadSanitizer has a fixed shadow layout and aborts ("unexpected memory mapping") on kernels that randomise
    mmap with more than 28 bits; without randomisation every mapping lands where it expects."""
    cmd = [shutil.which("setarch") or "setarch", platform.machine(), "-R"]
    try:
        ok = subprocess.run(cmd + ["true"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=30).returncode == 0
    except OSError:
        ok = False
    return cmd if ok else []


@pytest.mark.parametrize("san", ["thread", "address,undefined"])
def test_workers_under_sanitizer(san):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "workers_" + san.split(",")[0])
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=" + san, "-fno-omit-frame-pointer", "-pthread", SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1", ASAN_OPTIONS="detect_leaks=1")
        r = subprocess.run((_no_aslr() if san == "thread" else []) + [exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "workers ok" in r.stdout, r.stdout[-4000:]
