"""Who releases what inside the context (csrc/owned.hpp, csrc/rsreg_ctx.hpp), checked on the CPU: tests/cpp/ctx_owners.cpp is
compiled with plain g++ against its own counting definitions of the HIP calls the owners make -- no HIP runtime, no GPU --
and run under AddressSanitizer and UBSan.  A buffer, event or stream that deleting a context leaves behind, a handle released
twice, or a lane that a failed creation leaves half made fails it."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ctx_owners.cpp")
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_context_owners_under_sanitizer():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ctx_owners")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE, "-fsanitize=address,undefined",
                            "-fno-omit-frame-pointer", "-pthread", SRC, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "owners ok" in r.stdout, r.stdout[-4000:]
