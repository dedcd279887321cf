"""Builds the test model library whose device bodies bring the spatial VB kernels (tests/plugins/fwdmodel_spatial_models.hip)
for tests/test_device_spatial_model_registry.py and tests/test_device_spatial_model.py: hipcc for gfx950 against the public
headers, its five parts (FABBER_TEST_PART) side by side (five compile jobs, whatever the machine has), linked against
the host library and the engine. One build per test session; seconds[part] keeps how long each part took to compile."""
import atexit
import os
import shutil
import subprocess
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

from device_model_lib import HIP_FLAGS, INCLUDES, LIBDIR, ROOT, engine_built, hipcc  # noqa: F401 (engine_built: for the tests)

SRC = os.path.join(ROOT, "tests", "plugins", "fwdmodel_spatial_models.hip")
PARTS = (1, 2, 3, 4, 5)
MAX_JOBS = 16  # (a fixed bound, not the CPU count: the parts are few)

_BUILT = {}
seconds = {}


def build_library():
    """path of libfabber_models_spatial.so (built on first call)"""
    if "lib" in _BUILT:
        return _BUILT["lib"]
    cc = hipcc()
    out = tempfile.mkdtemp(prefix="fabber_spatial_models_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)  # (objects and library of this session)

    def compile_part(part):
        obj = os.path.join(out, "part%d.o" % part)
        t0 = time.perf_counter()
        p = subprocess.run([cc] + HIP_FLAGS + ["-DFABBER_TEST_PART=%d" % part] + INCLUDES + ["-c", SRC, "-o", obj],
                           capture_output=True, text=True)
        seconds[part] = time.perf_counter() - t0
        assert p.returncode == 0, p.stderr[-4000:]
        return obj

    with ThreadPoolExecutor(max_workers=min(len(PARTS), MAX_JOBS)) as ex:
        objs = list(ex.map(compile_part, PARTS))
    lib = os.path.join(out, "libfabber_models_spatial.so")
    p = subprocess.run([cc, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", lib] + objs
                       + ["-L", LIBDIR, "-lfabbercore_amd", "-lfabber_vb_hip", "-Wl,-rpath," + LIBDIR, "-Wl,--no-undefined"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    _BUILT["lib"] = lib
    return lib

