"""Builds the test model library with device bodies (tests/plugins/fwdmodel_device_models.hip) for
tests/test_device_model_registry.py and tests/test_device_model.py: hipcc for gfx950 against the public headers, its two
halves (FABBER_TEST_PART) side by side, linked against the host library and the engine. One build per test session."""
import atexit
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plugins", "fwdmodel_device_models.hip")
HOST = os.path.join(ROOT, "fabber_core_amd", "csrc", "host")
LIBDIR = os.path.join(ROOT, "fabber_core_amd", "lib")
HIP_FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-fast-math", "-Wno-deprecated-declarations"]
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", HOST, "-I", os.path.join(HOST, "fabber_core")]

_BUILT = {}


def engine_built():
    return os.path.exists(os.path.join(LIBDIR, "libfabber_vb_hip.so")) and os.path.exists(os.path.join(LIBDIR, "libfabbercore_amd.so"))


def hipcc():
    """hipcc, or an assertion: with the engine built, a missing compiler is a failure of the tests, not a reason to skip"""
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(exe), "hipcc not found: the model library with device bodies cannot be built"
    return exe


def build_library():
    """path of libfabber_models_device.so (built on first call)"""
    if "lib" in _BUILT:
        return _BUILT["lib"]
    cc = hipcc()
    out = tempfile.mkdtemp(prefix="fabber_device_models_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)  # (objects and library of this session)

    def compile_part(part):
        obj = os.path.join(out, "part%d.o" % part)
        p = subprocess.run([cc] + HIP_FLAGS + ["-DFABBER_TEST_PART=%d" % part] + INCLUDES + ["-c", SRC, "-o", obj], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-4000:]
        return obj

    with ThreadPoolExecutor(max_workers=2) as ex:
        objs = list(ex.map(compile_part, (1, 2)))
    lib = os.path.join(out, "libfabber_models_device.so")
    p = subprocess.run([cc, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", lib] + objs
                       + ["-L", LIBDIR, "-lfabbercore_amd", "-lfabber_vb_hip", "-Wl,-rpath," + LIBDIR, "-Wl,--no-undefined"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    _BUILT["lib"] = lib
    return lib
