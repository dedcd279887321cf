"""method=spatialvb for a model library's body against its yardsticks, same build, same process: the single exponential
over 50 timepoints, 10 iterations, on a 64 x 64 x 24 volume masked as in spatial_wide_rate.py (about 83 500 voxels), prior
M on the amplitude, as

    spatial<multiexp_sp,2>  the library's set-up kernel and second sweep (tests/plugins/fwdmodel_spatial_models.hip)
    spatial<exp,2>          the engine's built-in exponential model
    host route              the library's model evaluated on the host (option host-model), through fabber.run

Kernel time: fabber_vb_run_spatial_device on a series, an initial posterior and a result image that stay on the device
(the call returns when its stream has drained), after a warm-up of both tables; a run of 10 iterations and a run of 2
alternate over the rounds and over the two tables, the per-iteration figure is the difference of the medians / 8, so the
set-up (geometry, first linearisation) cancels. Whole call: fabber.run from host arrays to result images - the library's
device route and its host route - each twice, the second run is the one to quote. The two ratios DESIGN.md 3.5 quotes are
printed last: library / built-in (kernel time per iteration) and host route / library device route (whole call).

    python tools/measure/device_spatial_model_rate.py [--rounds 5] [--json PATH]
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

import device_model_lib
from fabber_core_amd import fabber, hiplib, vbabi
from fabber_core_amd.device import DeviceProblem

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

library = device_model_lib.build_spatial_library()
hiplib.load_model_library(library)
SHAPE, T, DT, ITERS, SHORT = (64, 64, 24), 50, 0.04, 10, 2
rng = np.random.default_rng(0)
mask = rng.random(SHAPE) < 0.85
coords = vbabi.grid_coords(SHAPE, mask)
V = coords.shape[1]
amp = 1.0 + 0.3 * np.sin(coords[0] / 3.0) * np.cos(coords[1] / 4.0) + 0.1 * np.sin(coords[2] / 2.0)
y = (amp[None, :] * np.exp(-1.0 * (np.arange(T) * DT)[:, None]) + rng.normal(0, 0.1, (T, V))).astype(np.float32)
sp = vbabi.SpatialHolder(coords)
results = []


def holders(iters):
    opts = dict(max_iterations=iters, param_overrides={"amp1": dict(type="M")})
    ref = vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=1, dt=DT, **opts)
    mvn = hiplib.initial_mvn(ref, y)
    ref = vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=1, dt=DT, init_mvn=mvn, **opts)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_sp", num_exps=1, dt=DT, init_mvn=mvn,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1), **opts)
    return {"spatial<multiexp_sp,2>": dev, "spatial<exp,2>": ref}


problems = {}
for iters in (ITERS, SHORT):
    for name, h in holders(iters).items():
        assert hiplib.spatial_kernel_name(h) == name, (hiplib.spatial_kernel_name(h), name)
        problems[name, iters] = DeviceProblem(h, y, "cuda:0")
for key, prob in problems.items():
    print("warm-up %s, %d iterations" % key, flush=True)
    prob.run_spatial(sp)  # (code objects, memory pool)
amps = {}
for name in ("spatial<multiexp_sp,2>", "spatial<exp,2>"):
    r = problems[name, ITERS].results()
    assert np.count_nonzero(r["status"]) < V // 1000
    amps[name] = float(np.mean(r["mvn"][6][r["status"] == 0]))  # (row 6: the first mean after the six covariance entries)
ms = {key: [] for key in problems}
for _ in range(args.rounds):
    for key, prob in problems.items():
        t0 = time.perf_counter()
        prob.run_spatial(sp)
        ms[key].append((time.perf_counter() - t0) * 1e3)
kernel = {}
for name in ("spatial<multiexp_sp,2>", "spatial<exp,2>"):
    long_ms, short_ms = float(np.median(ms[name, ITERS])), float(np.median(ms[name, SHORT]))
    kernel[name] = (long_ms - short_ms) / (ITERS - SHORT)
    results.append(dict(what="kernel", voxels=V, route=name, ms_per_iteration=kernel[name], ms_run_of_10=long_ms, ms_run_of_2=short_ms,
                        range_run_of_10=[min(ms[name, ITERS]), max(ms[name, ITERS])]))
    print("kernel  %6d voxels  %-24s %8.3f ms per iteration (run of %d: %.2f ms, range %.2f .. %.2f; run of %d: %.2f ms)  mean amp1 (Fabber space) %.5f"
          % (V, name, kernel[name], ITERS, long_ms, min(ms[name, ITERS]), max(ms[name, ITERS]), SHORT, short_ms, amps[name]), flush=True)
del problems

data = np.zeros(SHAPE + (T,), dtype=np.float32)
data[coords[0], coords[1], coords[2]] = y.T
call = {}
for rep in (1, 2):
    for name, extra, expect in (("spatial<multiexp_sp,2>", {}, "kernels spatial<multiexp_sp,2>"), ("host route", {"host-model": True}, "evaluated on the host")):
        opts = dict({"model": "multiexp_sp", "num-exps": 1, "dt": DT, "noise": "white", "method": "spatialvb", "max-iterations": ITERS,
                     "param-spatial-priors": "MN", "save-mean": True,
                     "allow-bad-voxels": True}, **extra)  # (a voxel of the mask without a neighbour has no M prior mean and fails)
        t0 = time.perf_counter()
        res = fabber.run(data, opts, mask=mask.astype(np.int32), model_libs=[library])
        dt = call[name] = time.perf_counter() - t0
        assert expect in res["log"], name
        results.append(dict(what="fabber.run", voxels=V, route=name, run=rep, seconds=dt))
        print("call %d  %6d voxels  %-24s %8.3f s  (%.1f ms per iteration, set-up included)  mean amp1 %.4f"
              % (rep, V, name, dt, dt / ITERS * 1e3, float(np.nanmean(res["mean_amp1"][mask]))), flush=True)
ratios = dict(what="ratios", voxels=V, library_over_builtin_kernel_time=kernel["spatial<multiexp_sp,2>"] / kernel["spatial<exp,2>"],
              host_route_over_device_route=call["host route"] / call["spatial<multiexp_sp,2>"])
results.append(ratios)
print("ratios  library / built-in (kernel time per iteration) %.3f   host route / library device route (whole call) %.2f"
      % (ratios["library_over_builtin_kernel_time"], ratios["host_route_over_device_route"]), flush=True)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(results, fh, indent=1)
