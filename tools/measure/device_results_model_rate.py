"""save-model-fit and save-residuals of a model library's body: the result-image kernel the library compiled around it
against the host loop, same build, same process. The single exponential over 50 timepoints, 10 iterations of voxelwise
VB, at 65 536 and 262 144 voxels, through whole fabber.run calls with both images asked for, as

    multiexp_res   lane kernels and a results entry (tests/plugins/fwdmodel_results_models.hip): model fit and
                   residuals from the device body (kernel postproc<multiexp_res>)
    multiexp_lane  the same lane kernels without a results entry (tests/plugins/fwdmodel_lane_models.hip): the fit is the
                   same, the two images come from the host loop - one thread, one EvaluateFabber per voxel

What is recorded are the laps of SaveEngineResults (FVB_HOST_TIMING=1 prints them on stderr, which is read back through
a file): "post-processing kernel (host pointers)" is the whole device call - uploads, kernel, downloads - and "model fit
and residuals on the host" is the loop. Each route runs once to warm up (code objects, memory pool, page faults of the
result arrays) and then --rounds times, the routes alternating; medians and ranges are printed, and last the ratio
DESIGN.md 3.5 quotes: (device call + host loop) of multiexp_lane over that of multiexp_res.

    python tools/measure/device_results_model_rate.py [--rounds 5] [--json PATH]
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import device_model_lib
import device_results_lib
from fabber_core_amd import fabber, hiplib

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

libraries = {"multiexp_res": device_results_lib.build_results_library(), "multiexp_lane": device_model_lib.build_lane_library()}
for path in libraries.values():
    hiplib.load_model_library(path)
assert "multiexp_res" in hiplib.device_results_models() and "multiexp_lane" not in hiplib.device_results_models()
T, DT, ITERS = 50, 0.04, 10
DEVICE_LAP, HOST_LAP = "post-processing kernel (host pointers)", "model fit and residuals on the host"
ROUTE_LINE = "model fit and residuals with the body"
os.environ["FVB_HOST_TIMING"] = "1"
LAP = re.compile(r"\[fabber host\] SaveEngineResults: (.*) ([0-9.]+) ms")


def timed_run(data, model):
    """one fabber.run; the laps of its SaveEngineResults in ms, the call in seconds, the result"""
    opts = {"model": model, "num-exps": 1, "dt": DT, "noise": "white", "method": "vb", "max-iterations": ITERS,
            "save-model-fit": True, "save-residuals": True}
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as fh:
        os.dup2(fh.fileno(), 2)
        try:
            t0 = time.perf_counter()
            res = fabber.run(data, opts, model_libs=[libraries[model]])
            seconds = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        fh.seek(0)
        text = fh.read()
    laps = {}
    for what, ms in LAP.findall(text):
        laps[what] = laps.get(what, 0.0) + float(ms)
    return laps, seconds, res


results = []
for shape in ((64, 64, 16), (64, 64, 64)):
    V = shape[0] * shape[1] * shape[2]
    rng = np.random.default_rng(V)
    amp, rate = rng.uniform(0.5, 1.5, shape), rng.uniform(0.6, 1.4, shape)
    data = (amp[..., None] * np.exp(-rate[..., None] * (np.arange(T) * DT)) + rng.normal(0, 0.1, shape + (T,))).astype(np.float32)
    fits = {}
    for model in libraries:  # warm-up, and what each route is
        laps, _, res = timed_run(data, model)
        assert "kernel lane<%s,2" % model in res["log"], model
        assert (ROUTE_LINE in res["log"]) == (model == "multiexp_res") and (any(k.startswith(HOST_LAP) for k in laps) == (model == "multiexp_lane"))
        fits[model] = res["modelfit"]
    print("%d voxels: max |fit of the body - fit of the host loop| %.3e" % (V, float(np.abs(fits["multiexp_res"] - fits["multiexp_lane"]).max())), flush=True)
    ms = {model: dict(device=[], host=[], save=[], call=[]) for model in libraries}
    for _ in range(args.rounds):
        for model in libraries:
            laps, seconds, _ = timed_run(data, model)
            ms[model]["device"].append(laps[DEVICE_LAP])
            ms[model]["host"].append(sum(v for k, v in laps.items() if k.startswith(HOST_LAP)))
            ms[model]["save"].append(sum(laps.values()))
            ms[model]["call"].append(seconds * 1e3)
    both = {}
    for model in libraries:
        med = {k: float(np.median(v)) for k, v in ms[model].items()}
        both[model] = med["device"] + med["host"]
        results.append(dict(what="fabber.run", voxels=V, model=model, rounds=args.rounds, median_ms=med,
                            range_ms={k: [min(v), max(v)] for k, v in ms[model].items()}))
        print("%7d voxels  %-14s device call %8.2f ms (%.2f .. %.2f)  host loop %9.2f ms (%.2f .. %.2f)  SaveEngineResults %9.2f ms  fabber.run %9.2f ms"
              % (V, model, med["device"], min(ms[model]["device"]), max(ms[model]["device"]), med["host"], min(ms[model]["host"]),
                 max(ms[model]["host"]), med["save"], med["call"]), flush=True)
    ratio = both["multiexp_lane"] / both["multiexp_res"]
    results.append(dict(what="ratio", voxels=V, host_loop_route_over_device_route=ratio))
    print("%7d voxels  model fit and residuals: host-loop route / device route %.1f" % (V, ratio), flush=True)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(results, fh, indent=1)
