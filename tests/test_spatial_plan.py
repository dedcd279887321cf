"""The planning half of the spatial VB host layer (fabber_core_amd/csrc/vb_spatial_plan.h: neighbour table, level order,
slab-major numbering, a_K segments, the z-slabs of a run on several devices) is plain C++17 without a HIP include:
tests/cpp/test_spatial_plan.cc is built with g++ alone, links no library and checks it against brute-force statements
of what it has to compute. CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fabber_core_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def test_spatial_plan(tmp_path):
    exe = str(tmp_path / "test_spatial_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_spatial_plan.cc"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
