"""Which engine entry point the host library calls, with which fvb_config: the host sources
(fabber_core_amd/csrc/host/*.cc) are compiled with a recording stand-in for the engine (tests/cpp/engine_recorder.cc)
and a driver (tests/cpp/test_engine_routing.cc) into one stand-alone program; what it prints - every engine call with
the contents of what it was handed (an fvb_config as its differences from the record before it), the techniques' log
lines, stage-timer laps and exceptions - has to equal tests/golden/engine_routing.txt line for line. The fixture was written by this program built against the host sources
as they were before the engine binding was shared between the techniques (FABBER_ROUTING_HOST_DIR names the
fabber_core_amd/csrc/host of another checkout to build against; FABBER_ROUTING_WRITE=1 writes the fixture). CPU only: g++,
no HIP, no engine library."""
import concurrent.futures
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.environ.get("FABBER_ROUTING_HOST_DIR") or os.path.join(ROOT, "fabber_core_amd", "csrc", "host")
CPP = os.path.join(ROOT, "tests", "cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_routing.txt")
FLAGS = ["-O1", "-std=c++17", "-Wall", "-Wno-unused-parameter", "-Wno-deprecated-declarations"] + os.environ.get("FABBER_ROUTING_FLAGS", "").split()

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def compile_one(job):
    src, obj = job
    cmd = ["g++"] + FLAGS + ["-I", HOST, "-I", os.path.join(HOST, "fabber_core"), "-c", src, "-o", obj]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return obj


def build(tmp_path):
    sources = sorted(glob.glob(os.path.join(HOST, "*.cc"))) + [os.path.join(CPP, "engine_recorder.cc"), os.path.join(CPP, "test_engine_routing.cc")]
    jobs = [(s, str(tmp_path / (os.path.basename(s) + ".o"))) for s in sources]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 2)) as ex:
        objs = list(ex.map(compile_one, jobs))
    exe = str(tmp_path / "test_engine_routing")
    p = subprocess.run(["g++"] + FLAGS + ["-o", exe] + objs + ["-ldl", "-lz", "-lpthread"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_engine_calls_and_configurations(tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert got and got[-1] == "==== end"
    if os.environ.get("FABBER_ROUTING_WRITE"):
        with open(GOLDEN, "w") as fh:
            fh.write(r.stdout)
    with open(GOLDEN) as fh:
        want = fh.read().splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d of the record differs from tests/golden/engine_routing.txt:\n  got:  %s\n  want: %s" % (i + 1, g, w)
    assert len(got) == len(want)
