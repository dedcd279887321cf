"""A model library's body on the lane-per-voxel kernels against its two yardsticks, same build, same process: the single
exponential over 50 timepoints, 10 iterations, at 65 536 and 262 144 voxels, as

    lane<multiexp_lane,2>   the library's lane kernels (tests/plugins/fwdmodel_lane_models.hip)
    wave<multiexp_lane>     the library's wave-per-voxel kernels (variant `wave`)
    lane<exp,2>             the engine's built-in exponential model

Kernel time: DeviceProblem (series and results stay on the device), device events around the enqueued runs, after a
warm-up of every route; the routes alternate over the rounds, the median and the range of the rounds are printed.
Whole call: fabber.run from host arrays to result images, each route twice, the second run is the one to quote.

    python tools/measure/device_lane_model_rate.py [--rounds 7] [--json PATH]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cases
import device_model_lib
from fabber_core_amd import fabber, hiplib, vbabi
from fabber_core_amd.device import DeviceProblem

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--json", default=None)
args = ap.parse_args()

library = device_model_lib.build_lane_library()
hiplib.load_model_library(library)
T, DT, ITS = 50, 0.04, 10
ROUTES = (("lane<multiexp_lane,2>", "plugin", "auto"), ("wave<multiexp_lane>", "plugin", "wave"), ("lane<exp,2>", "exp", "auto"))
results = []


def problems(V):
    ref, y = cases.exp_problem(V, T, 1, DT, seed=1, max_iterations=ITS)
    mvn = hiplib.initial_mvn(ref, y)
    ref, _ = cases.exp_problem(V, T, 1, DT, seed=1, max_iterations=ITS, init_mvn=mvn)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_lane", num_exps=1, dt=DT, init_mvn=mvn, max_iterations=ITS,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1))
    return {"plugin": dev, "exp": ref}, y


for V in (65536, 262144):
    holders, y = problems(V)
    probs = {}
    for name, which, variant in ROUTES:
        hiplib.set_variant(variant)
        probs[name] = DeviceProblem(holders[which], y, "cuda:0")
        assert probs[name].kernel == name, (probs[name].kernel, name)
        probs[name].run()  # warm-up: code object, pool memory
        torch.cuda.synchronize()
    means = {name: p.results()["mvn"][6:8].mean(axis=1) for name, p in probs.items()}
    ms = {name: [] for name in probs}
    for _ in range(args.rounds):
        for name, which, variant in ROUTES:
            hiplib.set_variant(variant)
            reps = 3 if name.startswith("wave") else 20  # (each window: tens of milliseconds and more)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                probs[name].run()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / reps)
    hiplib.set_variant("auto")
    for name in probs:
        med = float(np.median(ms[name]))
        results.append(dict(what="kernel", voxels=V, route=name, ms_median=med, ms_min=min(ms[name]), ms_max=max(ms[name]), voxels_per_s=V / med * 1e3))
        print("kernel  %7d voxels  %-22s %9.3f ms (range %.3f .. %.3f)  %12.0f voxels/s  mean (amp, log r) %s"
              % (V, name, med, min(ms[name]), max(ms[name]), V / med * 1e3, np.round(means[name], 5)), flush=True)
    del probs

    shape = (64, 64, V // 4096)
    data = np.ascontiguousarray(y.T.reshape(shape + (T,)))
    for rep in (1, 2):
        for name, which, variant in ROUTES:
            hiplib.set_variant(variant)
            opts = {"model": "multiexp_lane" if which == "plugin" else "exp", "num-exps": 1, "dt": DT, "noise": "white", "method": "vb",
                    "max-iterations": ITS, "save-mean": True}
            t0 = time.perf_counter()
            out = fabber.run(data, opts, model_libs=[library])
            dt = time.perf_counter() - t0
            assert "kernel " + name in out["log"], name
            results.append(dict(what="fabber.run", voxels=V, route=name, run=rep, seconds=dt, voxels_per_s=V / dt))
            print("call %d  %7d voxels  %-22s %9.3f s   %12.0f voxels/s  mean amp %.4f" % (rep, V, name, dt, V / dt, out["mean_amp1"].mean()), flush=True)
    hiplib.set_variant("auto")

if args.json:
    with open(args.json, "w") as fh:
        json.dump(results, fh, indent=1)
