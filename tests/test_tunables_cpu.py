"""csrc/tunables.hpp: every switch tunables_from_environment() reads is part of tunables_signature() (CPU only, g++).

tunables_refresh() -- what a new context calls -- re-reads the switches only when the signature has changed, so a switch the
signature leaves out keeps the value the process first read, and a test that sets it later runs the default path."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realsense-pointcloud_amd", "csrc")
HDR = os.path.join(CSRC, "tunables.hpp")
SRC = os.path.join(ROOT, "tests", "cpp", "tunables_sig.cpp")


def switch_names(diag):
    """The quoted RSREG_* names of the header's source text; those inside its `#ifdef RSREG_DIAG` blocks only when `diag`."""
    names, in_diag = set(), False
    for line in open(HDR).read().splitlines():
        s = line.strip()
        if s.startswith("#ifdef RSREG_DIAG"):
            in_diag = True
        elif s.startswith("#endif"):
            in_diag = False
        elif diag or not in_diag:
            names.update(re.findall(r'"(RSREG_[A-Z0-9_]+)"', line))
    return sorted(names)


def test_switch_names_are_found():
    plain, diag = switch_names(False), switch_names(True)
    assert {"RSREG_CELL_CAP", "RSREG_NO_BOX_CACHE", "RSREG_NO_NBR_FROM_TABLE", "RSREG_NDT_NO_WATCH"} <= set(plain)
    assert "RSREG_DEBUG_SKIP" in diag and "RSREG_DEBUG_SKIP" not in plain and set(plain) < set(diag)


@pytest.mark.parametrize("diag", [False, True], ids=["plain", "diag"])
def test_every_switch_changes_the_signature(diag):
    names = switch_names(diag)
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "tunables_sig")
        r = subprocess.run(["g++", "-std=c++17", "-O1", *(["-DRSREG_DIAG"] if diag else []), "-I", CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        r = subprocess.run([exe, *names], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    missing = re.findall(r"not in the signature: (\S+)", r.stdout)
    assert r.returncode == 0 and not missing and "signature ok: %d names" % len(names) in r.stdout, r.stdout[-3000:]
