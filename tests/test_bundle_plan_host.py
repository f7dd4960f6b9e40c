"""The bundle route (libjitsi_amd/csrc/bundle_plan.h: which kernels a bundle
runs, in which order, under which stage's timer) as checked without a GPU:
tools/bundle_plan_check compares plan_bundle with launch lists written out by
hand and sweeps it for the invariants every plan keeps, a program of its own
under AddressSanitizer + UBSan built from the check and the header alone."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rule_is_a_kernel_source_and_stands_alone():
    from libjitsi_amd import _native as N
    assert "bundle_plan.h" in N.KERNEL_SOURCES
    with open(os.path.join(ROOT, "libjitsi_amd", "csrc", "bundle_plan.h")) as fh:
        assert re.findall(r"#include\s*[<\"]([^>\"]*)", fh.read()) == ["stdint.h"]


def test_bundle_plan_check_builds_and_runs_clean(tmp_path):
    """tools/bundle_plan_check (the Makefile's recipe, built out of tree)."""
    with open(os.path.join(ROOT, "tools", "Makefile")) as fh:
        assert re.search(r"^bundle_plan_check: bundle_plan_check\.cpp .*bundle_plan\.h$", fh.read(), re.M)
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "bundle_plan_check")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "bundle_plan_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^bundle_plan_check: (\d+) cases, 0 failures$", r.stdout, re.M)
    assert m and int(m.group(1)) > 1000000, r.stdout
