"""method=spatialvb for a model library's body with more parameters than the lane kernels take (the wave-per-voxel spatial
kernels of include/fabber_device_spatial_wave_model.h) against the host route of the same library, same build, same
process: a 64^3 volume, 100 timepoints, 10 iterations, for

    multiexp_spw  num-exps=5 (10 parameters)   sum of exponentials, well-separated rates
    linear_spw    32 cosine regressors         the design in the body's constants block

(tests/plugins/fwdmodel_spatial_wave_models.hip), a spatial prior M on the first parameter.

Whole call: fabber.run from host arrays to result images - the library's device route (kernels spatial<NAME,wave>) and its
host route (option host-model: every iteration downloads the means, evaluates the model 2 P + 1 times per voxel on host
threads and uploads the linearisation; the behaviour before these kernels existed) - with 10 and with 2 iterations each. The
per-iteration figure is the difference / 8, so the set-up (geometry, initial posterior, first linearisation) cancels.

The sweeps of the device route one by one: fabber_vb_spatial_open on a series, an initial posterior and a result image that
stay on the device, then per iteration the a_K update, the first sweep (one launch per level) and the second sweep, each
timed with the stream drained after it (time.perf_counter around the call and torch.cuda.synchronize: host timers, launch
overhead included). The host family's second sweep cannot be started alone - it sits inside the engine's call between the
upload of the linearisation and the next download - so for the host route the tool gives the whole iteration only.

    python tools/measure/device_spatial_wave_rate.py [--models multiexp_spw,linear_spw] [--size 64] [--json PATH]

--patterns: instead of the above, the sweeps one by one under a noise pattern (the kernels of
include/fabber_device_spatial_wave_noise_model.h, tests/plugins/fwdmodel_spatial_wave_noise_models.hip): linear_spwn with 10 and
with 32 cosine regressors under 2 and under 8 precisions (spatial<linear_spwn,wave,phisN>) next to linear_spw of the same shape
under white noise with one precision (spatial<linear_spw,wave>), and two exponentials (4 parameters) under pattern 12 on the
wave kernels (multiexp_spwn), on the lane kernels (multiexp_spwn_both: spatial<multiexp_spwn_both,4,pattern2>, per-level first
sweep as the others) and under one precision (multiexp_spw) - same process, same job.

--ar: instead of the above, AR(1) noise with one echo (the kernels of include/fabber_device_spatial_wave_ar_model.h,
tests/plugins/fwdmodel_spatial_wave_ar_models.hip). The sweeps one by one: linear_spwa with 10 cosine regressors
(spatial<linear_spwa,wave,ar1>) next to linear_spw of the same shape under white noise with one precision, and two
exponentials (4 parameters) on the wave kernels (multiexp_spwa) and on the lane kernels (multiexp_spwa_both:
spatial<multiexp_spwa_both,4,ar1>, per-level first sweep as the others), and five exponentials (10 parameters) on the wave
kernels. Then the whole call for multiexp_spwa with three exponentials (6 parameters) under noise=ar: the device route
against the host route of the same library - the host route takes AR(1) noise up to 6 parameters and refuses it beyond, so
there is no host figure at 10.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import device_spatial_wave_ar_lib
import device_spatial_wave_lib
import device_spatial_wave_noise_lib
from fabber_core_amd import fabber, hiplib, vbabi
from fabber_core_amd.device import DeviceProblem
from fabber_core_amd.spatial_mgpu import _Run

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="multiexp_spw,linear_spw")
ap.add_argument("--size", type=int, default=64)
ap.add_argument("--times", type=int, default=100)
ap.add_argument("--json", default=None)
ap.add_argument("--skip-host-route", action="store_true")
ap.add_argument("--patterns", action="store_true")
ap.add_argument("--ar", action="store_true")
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()

library = device_spatial_wave_lib.build_spatial_wave_library()
hiplib.load_model_library(library)
SHAPE, T, ITERS, SHORT = (args.size,) * 3, args.times, args.iters, 2
coords = vbabi.grid_coords(SHAPE)
V = coords.shape[1]
sp = vbabi.SpatialHolder(coords)
rng = np.random.default_rng(0)
scale = 1.0 + 0.2 * np.sin(coords[0] / 5.0) * np.cos(coords[1] / 7.0) + 0.05 * np.sin(coords[2] / 3.0)
results = []
tmp = tempfile.mkdtemp(prefix="spw_rate_")


def multiexp():
    num, dt = 5, 0.006
    rates, amps = np.array([0.5, 3.0, 12.0, 40.0, 150.0]), np.array([1.0, 0.8, 0.6, 0.4, 0.3])
    t = np.arange(T) * dt
    y = (sum(amps[i] * scale[None, :] * np.exp(-rates[i] * t)[:, None] for i in range(num)) + rng.normal(0, 0.02, (T, V))).astype(np.float32)
    init = hiplib.initial_mvn(vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=num, dt=dt), y)
    nCov = (2 * num + 1) * (2 * num + 2) // 2
    for i in range(num):
        init[nCov + 2 * i], init[nCov + 2 * i + 1] = np.log(amps[i]), np.log(rates[i])
    holder = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_spw", num_exps=num, dt=dt, init_mvn=init,
                                max_iterations=ITERS, param_overrides={"amp1": dict(type="M")},
                                params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num))
    return y, holder, {"model": "multiexp_spw", "num-exps": num, "dt": dt, "param-spatial-priors": "M" + "N" * (2 * num - 1)}, "amp1"


def linear():
    P = 32
    X = np.cos(np.pi * np.arange(P)[None, :] * (np.arange(T)[:, None] + 0.5) / T)
    theta = np.stack([scale / (k + 1) for k in range(P)])
    y = (X @ theta + rng.normal(0, 0.1, (T, V))).astype(np.float32)
    params = vbabi.model_parameter_defaults(vbabi.MODEL_LINEAR, n_basis=P)
    ov = {"Parameter_1": dict(type="M")}
    init = hiplib.initial_mvn(vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, param_overrides=ov), y)
    n = P + 1
    for k in range(P):
        init[n * (n + 1) // 2 + k] = 1.0 / (k + 1)
    holder = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="linear_spw", constants=X, init_mvn=init, max_iterations=ITERS,
                                param_overrides=ov, params=params)
    basis = os.path.join(tmp, "design.mat")
    np.savetxt(basis, X)
    return y, holder, {"model": "linear_spw", "basis": basis, "param-spatial-priors": "M" + "N" * (P - 1)}, "Parameter_1"


def sweeps_one_by_one(name, holder, y, kernels=None, iters=None):
    """the device route's a_K update, first sweep and second sweep per iteration, the stream drained after each (iters: how
    many iterations, default --iters; the holder's max_iterations is the caller's)"""
    iters = iters or ITERS
    kernels = kernels or "spatial<%s,wave>" % name
    assert hiplib.spatial_kernel_name(holder) == kernels, (hiplib.spatial_kernel_name(holder), kernels)
    prob = DeviceProblem(holder, y, "cuda:0")
    prob.run_spatial(sp)  # warm-up: code objects, memory pool
    failed = int(np.count_nonzero(prob.results()["status"]))
    assert failed < max(1, V // 1000), failed
    ms = dict(ak=[], first=[], second=[])
    t_open = time.perf_counter()
    run = _Run(prob, sp, torch.cuda.current_stream(prob.device))
    torch.cuda.synchronize()
    ms_open = (time.perf_counter() - t_open) * 1e3
    try:
        for it in range(iters):
            for what, step in (("ak", None), ("first", lambda: run.sweep_levels(it, -2 ** 62, 2 ** 62)), ("second", lambda: run.sweep_noise(it))):
                t0 = time.perf_counter()
                if step is None:
                    if it > 0:
                        run.set_ak_sums(run.ak_sums())
                else:
                    step()
                torch.cuda.synchronize()
                ms[what].append((time.perf_counter() - t0) * 1e3)
    finally:
        run.close()
    out = dict(what="sweeps", route=kernels, voxels=V, failed_voxels=failed, timepoints=T, parameters=holder.cfg.n_params, ms_open_with_set_up=ms_open,
               **{"ms_%s_median" % k: float(np.median(v[1:])) for k, v in ms.items()}, **{"ms_%s_all" % k: v for k, v in ms.items()})
    results.append(out)
    print("sweeps  %-28s %7d voxels T=%d P=%d: open + set-up %.1f ms; per iteration (median of iterations 2..%d) a_K %.2f ms, first sweep %.2f ms, "
          "second sweep %.2f ms" % (out["route"], V, T, holder.cfg.n_params, ms_open, iters, out["ms_ak_median"], out["ms_first_median"],
                                    out["ms_second_median"]), flush=True)
    out["ms_iteration_median"] = float(np.median(np.array(ms["ak"][1:]) + np.array(ms["first"][1:]) + np.array(ms["second"][1:])))
    print("sweeps  %-28s per spatial iteration %.2f ms" % (out["route"], out["ms_iteration_median"]), flush=True)
    del prob


def whole_calls(name, y, model_opts, first, noise="white", kernels=None, library=library, ITERS=ITERS):
    data = np.zeros(SHAPE + (T,), dtype=np.float32)
    data[coords[0], coords[1], coords[2]] = y.T
    secs = {}
    routes = [("device route", {}, "kernels " + (kernels or "spatial<%s,wave>" % name))]
    if not args.skip_host_route:
        routes.append(("host route", {"host-model": True}, "the model is evaluated on the host"))
    for route, extra, expect in routes:
        # (the device route's first call warms it up - code objects, memory pool - and is repeated; the host route's calls are
        # long against that)
        for iters in ((SHORT, SHORT, ITERS) if not extra else (SHORT, ITERS)):
            opts = dict({"noise": noise, "method": "spatialvb", "max-iterations": iters, "save-mean": True, "allow-bad-voxels": True},
                        **model_opts, **extra)
            t0 = time.perf_counter()
            res = fabber.run(data, opts, model_libs=[library])
            secs[route, iters] = time.perf_counter() - t0
            assert expect in res["log"], (route, res["log"][-2000:])
            print("call    %-28s %-12s %2d iterations %8.3f s   mean %s %.5f" % (name, route, iters, secs[route, iters], first,
                                                                                float(np.nanmean(res["mean_" + first]))), flush=True)
        per_it = (secs[route, ITERS] - secs[route, SHORT]) / (ITERS - SHORT)
        results.append(dict(what="fabber.run", model=name, route=route, voxels=V, timepoints=T, iterations_long_run=ITERS, seconds_run_of_10=secs[route, ITERS],
                            seconds_run_of_2=secs[route, SHORT], seconds_per_iteration=per_it))
        print("call    %-28s %-12s %.3f s per iteration (run of %d minus run of %d, / %d)" % (name, route, per_it, ITERS, SHORT, ITERS - SHORT), flush=True)
    if not args.skip_host_route:
        ratio = dict(what="ratios", model=name, whole_call_host_over_device=secs["host route", ITERS] / secs["device route", ITERS],
                     per_iteration_host_over_device=((secs["host route", ITERS] - secs["host route", SHORT])
                                                     / max(1e-9, secs["device route", ITERS] - secs["device route", SHORT])))
        results.append(ratio)
        print("ratios  %-28s host route / device route: whole call of %d iterations %.2f, per iteration %.2f"
              % (name, ITERS, ratio["whole_call_host_over_device"], ratio["per_iteration_host_over_device"]), flush=True)


def linear_pattern(P, pattern):
    """P cosine regressors, a prior M on the first; pattern None: linear_spw under one precision, else linear_spwn"""
    X = np.cos(np.pi * np.arange(P)[None, :] * (np.arange(T)[:, None] + 0.5) / T)
    theta = np.stack([scale / (k + 1) for k in range(P)])
    y = (X @ theta + np.random.default_rng(P).normal(0, 0.1, (T, V))).astype(np.float32)
    kw = dict(param_overrides={"Parameter_1": dict(type="M")}, **({"noise_pattern": pattern} if pattern else {}))
    init = hiplib.initial_mvn(vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, **kw), y)
    n = P + (len(set(pattern)) if pattern else 1)
    for k in range(P):
        init[n * (n + 1) // 2 + k] = 1.0 / (k + 1)
    name = "linear_spwn" if pattern else "linear_spw"
    return name, y, vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, constants=X, init_mvn=init, max_iterations=ITERS,
                                       params=vbabi.model_parameter_defaults(vbabi.MODEL_LINEAR, n_basis=P), **kw)


def biexp_pattern(name, pattern):
    num, dt = 2, 0.006
    rates, amps = np.array([0.5, 12.0]), np.array([1.0, 0.6])
    t = np.arange(T) * dt
    y = (sum(amps[i] * scale[None, :] * np.exp(-rates[i] * t)[:, None] for i in range(num))
         + np.random.default_rng(4).normal(0, 0.02, (T, V))).astype(np.float32)
    kw = dict(num_exps=num, dt=dt, param_overrides={"amp1": dict(type="M")}, **({"noise_pattern": pattern} if pattern else {}))
    init = hiplib.initial_mvn(vbabi.build_config(vbabi.MODEL_EXP, V, T, **kw), y)
    n = 2 * num + (len(set(pattern)) if pattern else 1)
    for i in range(num):
        init[n * (n + 1) // 2 + 2 * i], init[n * (n + 1) // 2 + 2 * i + 1] = np.log(amps[i]), np.log(rates[i])
    return y, vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, init_mvn=init, max_iterations=ITERS,
                                 params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num), **kw)


if args.patterns:
    hiplib.load_model_library(device_spatial_wave_noise_lib.build_spatial_wave_noise_library())
    os.environ["FVB_SPATIAL_PER_LEVEL"] = "1"  # (the lane route's first sweep as the wave routes': one launch per level)
    for P in (10, 32):
        for pattern in (None, "12", "12345678"):
            name, y, holder = linear_pattern(P, pattern)
            sweeps_one_by_one(name, holder, y, None if pattern is None else "spatial<%s,wave,phis%d>" % (name, len(pattern)))
            if args.json:
                with open(args.json, "w") as fh:
                    json.dump(results, fh, indent=1)
    for name, pattern, kernels in (("multiexp_spw", None, None), ("multiexp_spwn", "12", "spatial<multiexp_spwn,wave,phis2>"),
                                   ("multiexp_spwn_both", "12", "spatial<multiexp_spwn_both,4,pattern2>")):
        y, holder = biexp_pattern(name, pattern)
        sweeps_one_by_one(name, holder, y, kernels)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(results, fh, indent=1)
    sys.exit(0)

def ar_image(white, P, holder):
    return device_spatial_wave_ar_lib.ar_image(white, P, holder)


if args.ar:
    AR = device_spatial_wave_ar_lib.AR
    ar_library = device_spatial_wave_ar_lib.build_spatial_wave_ar_library()
    hiplib.load_model_library(ar_library)
    os.environ["FVB_SPATIAL_PER_LEVEL"] = "1"  # (the lane route's first sweep as the wave routes': one launch per level)
    # 10 cosine regressors: one precision on linear_spw, AR(1) on linear_spwa
    name, y, holder = linear_pattern(10, None)
    sweeps_one_by_one(name, holder, y)
    P = 10
    X = np.cos(np.pi * np.arange(P)[None, :] * (np.arange(T)[:, None] + 0.5) / T)  # (linear_pattern's design and series)
    kw = dict(param_overrides={"Parameter_1": dict(type="M")})
    init = ar_image(hiplib.initial_mvn(vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, **kw), y), P,
                    vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, **kw, **AR))
    n = P + 3
    for k in range(P):
        init[n * (n + 1) // 2 + k] = 1.0 / (k + 1)
    holder = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="linear_spwa", constants=X, init_mvn=init, max_iterations=ITERS,
                                params=vbabi.model_parameter_defaults(vbabi.MODEL_LINEAR, n_basis=P), **kw, **AR)
    sweeps_one_by_one("linear_spwa", holder, y, "spatial<linear_spwa,wave,ar1>")

    # The exponential fits under AR(1) noise run EXP_ITERS iterations: with more, most voxels of these series (white noise
    # in the data) stop with a status - in the CPU oracle as on the device, 80 % of them after 10 iterations of the two
    # exponentials - and leave the sweeps, so a later iteration times another problem.
    EXP_ITERS = min(ITERS, 4)

    def exp_ar(name, num, dt=0.006):
        rates, amps = np.array([0.5, 3.0, 12.0, 40.0, 150.0])[:num], np.array([1.0, 0.8, 0.6, 0.4, 0.3])[:num]
        if num == 2:
            rates, amps = np.array([0.5, 12.0]), np.array([1.0, 0.6])
        t = np.arange(T) * dt
        y = (sum(amps[i] * scale[None, :] * np.exp(-rates[i] * t)[:, None] for i in range(num))
             + np.random.default_rng(4).normal(0, 0.02, (T, V))).astype(np.float32)
        kw = dict(num_exps=num, dt=dt, param_overrides={"amp1": dict(type="M")})
        init = ar_image(hiplib.initial_mvn(vbabi.build_config(vbabi.MODEL_EXP, V, T, **kw), y), 2 * num,
                        vbabi.build_config(vbabi.MODEL_EXP, V, T, **kw, **AR))
        n = 2 * num + 3
        for i in range(num):
            init[n * (n + 1) // 2 + 2 * i], init[n * (n + 1) // 2 + 2 * i + 1] = np.log(amps[i]), np.log(rates[i])
        return y, vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, init_mvn=init, max_iterations=EXP_ITERS,
                                     params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num), **kw, **AR)

    for name, kernels in (("multiexp_spwa", "spatial<multiexp_spwa,wave,ar1>"), ("multiexp_spwa_both", "spatial<multiexp_spwa_both,4,ar1>")):
        y, holder = exp_ar(name, 2)
        sweeps_one_by_one(name, holder, y, kernels, iters=EXP_ITERS)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(results, fh, indent=1)
    y, holder = exp_ar("multiexp_spwa", 5)
    sweeps_one_by_one("multiexp_spwa", holder, y, "spatial<multiexp_spwa,wave,ar1>", iters=EXP_ITERS)
    y, holder = exp_ar("multiexp_spwa", 3)
    sweeps_one_by_one("multiexp_spwa", holder, y, "spatial<multiexp_spwa,wave,ar1>", iters=EXP_ITERS)
    whole_calls("multiexp_spwa", y, {"model": "multiexp_spwa", "num-exps": 3, "dt": 0.006, "param-spatial-priors": "M" + "N" * 5}, "amp1",
                noise="ar", kernels="spatial<multiexp_spwa,wave,ar1>", library=ar_library, ITERS=EXP_ITERS)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(results, fh, indent=1)
    sys.exit(0)

for name in args.models.split(","):
    y, holder, model_opts, first = {"multiexp_spw": multiexp, "linear_spw": linear}[name]()
    sweeps_one_by_one(name, holder, y)
    whole_calls(name, y, model_opts, first)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(results, fh, indent=1)
