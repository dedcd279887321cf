"""method=spatialvb for a model library's body under AR(1) noise and a noise pattern, and with per-voxel supplementary
data, against its yardsticks, same build, same process: 50 timepoints, 10 iterations, on the 64 x 64 x 24 volume of
device_spatial_model_rate.py (about 83 500 voxels), prior M on the amplitude, as

    spatial<multiexp_spn,2,ar1>       the library's set-up kernel and second sweep (tests/plugins/fwdmodel_spatial_noise_models.hip)
    spatial<exp,2,ar1>                the engine's built-in exponential model
    spatial<multiexp_spn,2,pattern2>  ... under noise-pattern 12
    spatial<exp,2,pattern2>
    host route                        the library's model evaluated on the host (option host-model), through fabber.run:
                                      multiexp_spn under noise=ar, and suppconv_sp (a convolution with the voxel's input
                                      curve, 50 supplementary rows) under white noise

Kernel time: fabber_vb_run_spatial_device on a series, an initial posterior and a result image that stay on the device (the
call returns when its stream has drained), after a warm-up of every table; a run of 10 iterations and a run of 2 alternate
over the rounds and over the tables, the per-iteration figure is the difference of the medians / 8, so the set-up
(geometry, first linearisation) cancels; the range of the runs of 10 is printed next to it. Whole call: fabber.run from host
arrays to result images - the library's device route and its host route - each twice, the second run is the one to quote.
The ratios DESIGN.md 3.5 quotes are printed last.

    python tools/measure/device_spatial_noise_rate.py [--rounds 5] [--json PATH]
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
from test_device_model import initial_mvn

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

library = device_model_lib.build("fwdmodel_spatial_noise_models.hip", (1, 2, 3, 4, 5), "libfabber_models_spatial_noise.so")
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
NOISES = {"ar1": dict(noise=vbabi.NOISE_AR1, num_echoes=1), "pattern2": dict(noise_pattern="12")}


def holders(iters, tag):
    opts = dict(max_iterations=iters, param_overrides={"amp1": dict(type="M")}, **NOISES[tag])
    ref = vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=1, dt=DT, **opts)
    mvn = initial_mvn(ref, y)
    ref = vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=1, dt=DT, init_mvn=mvn, **opts)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_spn", num_exps=1, dt=DT, init_mvn=mvn,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1), **opts)
    return {"spatial<multiexp_spn,2,%s>" % tag: dev, "spatial<exp,2,%s>" % tag: ref}


problems = {}
for tag in NOISES:
    for iters in (ITERS, SHORT):
        for name, h in holders(iters, tag).items():
            assert hiplib.spatial_kernel_name(h) == name, (hiplib.spatial_kernel_name(h), name)
            problems[name, iters] = DeviceProblem(h, y, "cuda:0")
for key, prob in problems.items():
    print("warm-up %s, %d iterations" % key, flush=True)
    prob.run_spatial(sp)  # (code objects, memory pool)
names = sorted({name for name, _ in problems})
for name in names:
    r = problems[name, ITERS].results()
    assert np.count_nonzero(r["status"]) < V // 1000, name
ms = {key: [] for key in problems}
for _ in range(args.rounds):
    for key, prob in problems.items():
        t0 = time.perf_counter()
        prob.run_spatial(sp)
        ms[key].append((time.perf_counter() - t0) * 1e3)
kernel = {}
for name in names:
    long_ms, short_ms = float(np.median(ms[name, ITERS])), float(np.median(ms[name, SHORT]))
    kernel[name] = (long_ms - short_ms) / (ITERS - SHORT)
    results.append(dict(what="kernel", voxels=V, route=name, ms_per_iteration=kernel[name], ms_run_of_10=long_ms, ms_run_of_2=short_ms,
                        range_run_of_10=[min(ms[name, ITERS]), max(ms[name, ITERS])], range_run_of_2=[min(ms[name, SHORT]), max(ms[name, SHORT])]))
    print("kernel  %6d voxels  %-34s %8.3f ms per iteration (run of %d: %.2f ms, range %.2f .. %.2f; run of %d: %.2f ms, range %.2f .. %.2f)"
          % (V, name, kernel[name], ITERS, long_ms, min(ms[name, ITERS]), max(ms[name, ITERS]), SHORT, short_ms, min(ms[name, SHORT]),
             max(ms[name, SHORT])), flush=True)
del problems


def volume_of(rows):
    vol = np.zeros(SHAPE + (rows.shape[0],), dtype=np.float32)
    vol[coords[0], coords[1], coords[2]] = rows.T
    return vol


# the convolution model: a bump per voxel whose onset differs from voxel to voxel, amplitudes of order 100 with noise of 2
DT_SUPP = 0.25
onset = rng.integers(0, 6, V)
t = np.arange(T)[:, None]
supp = np.where(t >= onset, rng.uniform(0.5, 2.0, V) * np.exp(-0.5 * ((t - onset - 2.0) / 1.5) ** 2), 0.0)
rate = rng.uniform(0.5, 1.5, V)
clean = np.zeros((T, V))
for i in range(T):
    for s in range(i + 1):
        clean[i] += supp[s] * np.exp(-rate * ((i - s) * DT_SUPP))
y_supp = (100.0 * amp * clean + rng.normal(0, 2.0, (T, V))).astype(np.float32)
CALLS = (("multiexp_spn", "ar", "spatial<multiexp_spn,2,ar1>", volume_of(y), None, {"num-exps": 1, "dt": DT}, "mean_amp"),
         ("suppconv_sp", "white", "spatial<suppconv_sp,2>", volume_of(y_supp), {"suppdata": volume_of(supp)}, {"dt": DT_SUPP}, "mean_amp"))
call = {}
for rep in (1, 2):
    for model, noise, kernels, data, extra_data, model_opts, mean in CALLS:
        for route, extra, expect in ((kernels, {}, "kernels " + kernels), ("host route", {"host-model": True}, "evaluated on the host")):
            opts = dict({"model": model, "noise": noise, "method": "spatialvb", "max-iterations": ITERS, "param-spatial-priors": "MN",
                         "save-mean": True,
                         "allow-bad-voxels": True}, **model_opts, **extra)  # (a voxel of the mask without a neighbour has no M prior mean and fails)
            t0 = time.perf_counter()
            res = fabber.run(data, opts, mask=mask.astype(np.int32), extra_data=extra_data, model_libs=[library])
            dt = call[model, route] = time.perf_counter() - t0
            assert expect in res["log"], (model, route)
            results.append(dict(what="fabber.run", voxels=V, model=model, noise=noise, route=route, run=rep, seconds=dt))
            print("call %d  %6d voxels  %-12s %-5s %-30s %8.3f s  (%.1f ms per iteration, set-up included)  mean amp %.4f"
                  % (rep, V, model, noise, route, dt, dt / ITERS * 1e3, float(np.nanmean(res[mean][mask]))), flush=True)
ratios = dict(what="ratios", voxels=V,
              library_over_builtin_kernel_time_ar1=kernel["spatial<multiexp_spn,2,ar1>"] / kernel["spatial<exp,2,ar1>"],
              library_over_builtin_kernel_time_pattern2=kernel["spatial<multiexp_spn,2,pattern2>"] / kernel["spatial<exp,2,pattern2>"],
              host_route_over_device_route_multiexp_ar=call["multiexp_spn", "host route"] / call["multiexp_spn", "spatial<multiexp_spn,2,ar1>"],
              host_route_over_device_route_suppconv_white=call["suppconv_sp", "host route"] / call["suppconv_sp", "spatial<suppconv_sp,2>"])
results.append(ratios)
print("ratios  library / built-in (kernel time per iteration): ar1 %.3f  pattern2 %.3f   host route / library device route (whole call): "
      "multiexp_spn under ar %.2f  suppconv_sp under white noise %.2f"
      % (ratios["library_over_builtin_kernel_time_ar1"], ratios["library_over_builtin_kernel_time_pattern2"],
         ratios["host_route_over_device_route_multiexp_ar"], ratios["host_route_over_device_route_suppconv_white"]), flush=True)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(results, fh, indent=1)
