"""The initial posterior of a model library's body: the kernel the library compiled around its init_posterior
(include/fabber_device_init_model.h) against the host loop of Vb::BuildInitialMvn, same build, same session. The single
exponential over 50 timepoints, 10 iterations of voxelwise VB, at 65 536 and 262 144 voxels, through whole fabber.run
calls of tests/plugins/fwdmodel_init_models.hip built twice:

    with     all its parts: multiexp_init has an init entry, the image is written on the device inside the engine call
    without  the same source without the part that holds the FABBER_DEVICE_INIT_MODEL lines: the same lane kernels fit,
             the image comes from the host loop - one thread, PassData + GetInitialPosterior + a strided scatter per voxel

Each (route, size) is a process of its own under its own time limit; it runs twice and reports the SECOND run (code
objects loaded, memory pool filled, result arrays faulted in): the whole call, and the laps of Vb::DoCalculations that
FVB_HOST_TIMING=1 prints on stderr - "initial posterior ..." is the step itself on either route (on the device route the
host does nothing there: the kernel runs inside the "engine" lap), "engine" is the engine call. One more process times
the kernel alone with events (fabber_vb_init_posterior_device, median of 20 launches), with the bytes it moves per voxel.

    python tools/measure/device_init_model_rate.py [--rounds 3] [--json PATH]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

T, DT, ITERS = 50, 0.04, 10
SHAPES = ((64, 64, 16), (64, 64, 64))
MODEL = "multiexp_init"
LAP = re.compile(r"\[fabber host\] Vb::DoCalculations: (.*) ([0-9.]+) ms")
CHILD_SECONDS = 300  # the time limit of one child: a whole fabber.run of 262 144 voxels takes well under a second


def volume(shape):
    V = shape[0] * shape[1] * shape[2]
    rng = np.random.default_rng(V)
    amp, rate = rng.uniform(0.5, 1.5, shape), rng.uniform(0.6, 1.4, shape)
    return (amp[..., None] * np.exp(-rate[..., None] * (np.arange(T) * DT)) + rng.normal(0, 0.1, shape + (T,))).astype(np.float32)


def child_run(library, shape, with_entry):
    """two fabber.run calls; the second one's call time and laps as one JSON line"""
    from fabber_core_amd import fabber, hiplib
    os.environ["FVB_HOST_TIMING"] = "1"
    hiplib.load_model_library(library)
    assert (MODEL in hiplib.device_init_models()) == with_entry
    data = volume(shape)
    opts = {"model": MODEL, "num-exps": 1, "dt": DT, "noise": "white", "method": "vb", "max-iterations": ITERS, "save-mean": True}
    for _ in range(2):
        sys.stderr.flush()
        saved = os.dup(2)
        with tempfile.TemporaryFile(mode="w+") as fh:
            os.dup2(fh.fileno(), 2)
            try:
                t0 = time.perf_counter()
                res = fabber.run(data, opts, model_libs=[library])
                seconds = time.perf_counter() - t0
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            fh.seek(0)
            text = fh.read()
    assert "kernel lane<%s,2" % MODEL in res["log"]
    assert ("kernel init<%s>" % MODEL in res["log"]) == with_entry
    laps = {}
    for what, ms in LAP.findall(text):
        laps[what] = laps.get(what, 0.0) + float(ms)
    init = sum(v for k, v in laps.items() if k.startswith("initial posterior"))
    print(json.dumps(dict(call_ms=seconds * 1e3, init_ms=init, engine_ms=laps.get("engine", float("nan")), laps=laps)))


def child_kernel(library):
    """the kernel alone at both sizes: median of 20 launches between events, after 3 to warm up"""
    import ctypes as C
    import torch
    from fabber_core_amd import hiplib, vbabi
    hiplib.load_model_library(library)
    out = []
    for shape in SHAPES:
        V = shape[0] * shape[1] * shape[2]
        h = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=MODEL, num_exps=1, dt=DT,
                               params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1))
        y = torch.from_numpy(volume(shape).reshape(V, T).T.copy()).to("cuda:0")
        # (the C entry point with a configuration that is on the device already: nothing but the launch between the events)
        d, keep = hiplib.device_config(h, y.device, False)
        img = torch.empty((h.n_mvn_rows, V), dtype=torch.float64, device=y.device)
        stream = torch.cuda.current_stream(y.device)
        ms = []
        for i in range(23):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = hiplib.lib().fabber_vb_init_posterior_device(C.byref(d), y.data_ptr(), img.data_ptr(), C.c_void_p(stream.cuda_stream))
            b.record()
            torch.cuda.synchronize()
            assert rc == 0, hiplib.lib().fabber_vb_last_error().decode()
            if i >= 3:
                ms.append(a.elapsed_time(b))
        # one sample of the series read (this body reads y(0) only: one float), rows of the image written
        out.append(dict(voxels=V, kernel_ms=float(np.median(ms)), range_ms=[min(ms), max(ms)],
                        bytes_written_per_voxel=8 * h.n_mvn_rows, bytes_read_per_voxel=4))
    print(json.dumps(out))


def spawn(args, seconds=CHILD_SECONDS):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=seconds)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)  # library, voxels along z, with entry (0 / 1)
    ap.add_argument("--kernel", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child_run(args.child[0], (64, 64, int(args.child[1])), args.child[2] == "1")
    if args.kernel:
        return child_kernel(args.kernel)
    import device_init_lib
    import device_model_lib
    libraries = {"with": device_init_lib.build_init_library(),
                 "without": device_model_lib.build("fwdmodel_init_models.hip", device_init_lib.PARTS[:-1], "libfabber_models_init_without.so")}
    results = []
    for shape in SHAPES:
        V = shape[0] * shape[1] * shape[2]
        runs = {route: [] for route in libraries}
        for _ in range(args.rounds):
            for route, path in libraries.items():  # (the routes alternate)
                runs[route].append(spawn(["--child", path, str(shape[2]), "1" if route == "with" else "0"]))
        med = {}
        for route in libraries:
            med[route] = {k: float(np.median([r[k] for r in runs[route]])) for k in ("call_ms", "init_ms", "engine_ms")}
            rng = {k: [min(r[k] for r in runs[route]), max(r[k] for r in runs[route])] for k in ("call_ms", "init_ms", "engine_ms")}
            results.append(dict(what="fabber.run", voxels=V, route=route, rounds=args.rounds, median_ms=med[route], range_ms=rng))
            print("%7d voxels  %-7s entry  fabber.run %8.2f ms (%.2f .. %.2f)  initial posterior lap %8.2f ms (%.2f .. %.2f)  engine lap %8.2f ms"
                  % (V, route, med[route]["call_ms"], rng["call_ms"][0], rng["call_ms"][1], med[route]["init_ms"], rng["init_ms"][0],
                     rng["init_ms"][1], med[route]["engine_ms"]), flush=True)
        print("%7d voxels  whole call without / with the entry: %.2f" % (V, med["without"]["call_ms"] / med["with"]["call_ms"]), flush=True)
    for k in spawn(["--kernel", libraries["with"]]):
        results.append(dict(what="kernel", **k))
        print("%7d voxels  kernel init<%s> %.3f ms (%.3f .. %.3f), %d bytes written and %d read per voxel"
              % (k["voxels"], MODEL, k["kernel_ms"], k["range_ms"][0], k["range_ms"][1], k["bytes_written_per_voxel"], k["bytes_read_per_voxel"]),
              flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
