"""Builds the test model libraries with device bodies (tests/plugins/fwdmodel_*_models.hip) for the tests and the measuring
tools of those bodies: hipcc for gfx950 against the public headers, the parts of a source (FABBER_TEST_PART) side by
side, linked against the host library and the engine. One build of a library per test session; seconds[library][part]
keeps how long each part took to compile."""
import atexit
import os
import shutil
import subprocess
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "fabber_core_amd", "csrc", "host")
LIBDIR = os.path.join(ROOT, "fabber_core_amd", "lib")
HIP_FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-fast-math", "-Wno-deprecated-declarations"]
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", HOST, "-I", os.path.join(HOST, "fabber_core")]

MAX_JOBS = 16  # (a fixed bound, not the CPU count: the parts are few)

_BUILT = {}
seconds = {}


def engine_built():
    return os.path.exists(os.path.join(LIBDIR, "libfabber_vb_hip.so")) and os.path.exists(os.path.join(LIBDIR, "libfabbercore_amd.so"))


def hipcc():
    """hipcc, or an assertion: with the engine built, a missing compiler is a failure of the tests, not a reason to skip"""
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(exe), "hipcc not found: the model library with device bodies cannot be built"
    return exe


def build(source, parts, library):
    """path of `library` (libNAME.so), built on first call from tests/plugins/`source`, one compile job per part"""
    if library in _BUILT:
        return _BUILT[library]
    cc = hipcc()
    out = tempfile.mkdtemp(prefix=library.replace(".so", "_"))
    atexit.register(shutil.rmtree, out, ignore_errors=True)  # (objects and library of this session)
    src = os.path.join(ROOT, "tests", "plugins", source)
    seconds[library] = {}

    def compile_part(part):
        obj = os.path.join(out, "part%d.o" % part)
        t0 = time.perf_counter()
        p = subprocess.run([cc] + HIP_FLAGS + ["-DFABBER_TEST_PART=%d" % part] + INCLUDES + ["-c", src, "-o", obj],
                           capture_output=True, text=True)
        seconds[library][part] = time.perf_counter() - t0
        assert p.returncode == 0, p.stderr[-4000:]
        return obj

    with ThreadPoolExecutor(max_workers=min(len(parts), MAX_JOBS)) as ex:
        objs = list(ex.map(compile_part, parts))
    lib = os.path.join(out, library)
    p = subprocess.run([cc, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", lib] + objs
                       + ["-L", LIBDIR, "-lfabbercore_amd", "-lfabber_vb_hip", "-Wl,-rpath," + LIBDIR, "-Wl,--no-undefined"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    _BUILT[library] = lib
    return lib


def build_library():
    """the wave-per-voxel bodies alone (multiexp_dev, invrec)"""
    return build("fwdmodel_device_models.hip", (1, 2), "libfabber_models_device.so")


def build_lane_library():
    """bodies with their lane-per-voxel kernels (multiexp_lane, invrec_lane)"""
    return build("fwdmodel_lane_models.hip", (1, 2, 3, 4, 5), "libfabber_models_lane.so")


def build_nlls_library():
    """bodies with their NLLS minimisers (multiexp_nlls, invrec_nlls)"""
    return build("fwdmodel_nlls_models.hip", (1, 2, 3, 4, 5), "libfabber_models_nlls.so")


def build_spatial_library():
    """bodies with their spatial VB kernels (multiexp_sp, invrec_sp)"""
    return build("fwdmodel_spatial_models.hip", (1, 2, 3, 4, 5), "libfabber_models_spatial.so")
