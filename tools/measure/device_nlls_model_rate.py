"""method=nlls for a model library's body against its yardsticks, same build, same process: the single exponential over 50
timepoints at 65 536 and 262 144 voxels, as

    nlls<multiexp_nlls,2>     the library's lane-per-voxel minimiser (tests/plugins/fwdmodel_nlls_models.hip)
    nlls_wave<multiexp_nlls>  the library's wave-per-voxel minimiser (variant `wave`)
    nlls<exp,2>               the engine's built-in exponential model
    host route                the library's model evaluated on the host (option host-model), through fabber.run

Kernel time: fabber_nlls_run_device on a series and a result image that stay on the device, device events around the
enqueued runs, after a warm-up of every route; the routes alternate over the rounds, the median and the range of the
rounds are printed. Whole call: fabber.run from host arrays to result images - the library's device route and its host
route - each twice, the second run is the one to quote. The two ratios DESIGN.md 3.6 quotes are printed last: library
lane / built-in lane (kernel time) and library device route / host route (whole call).

    python tools/measure/device_nlls_model_rate.py [--rounds 7] [--json PATH]
"""
import argparse
import ctypes as C
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

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--json", default=None)
args = ap.parse_args()

library = device_model_lib.build_nlls_library()
hiplib.load_model_library(library)
T, DT = 50, 0.04
ROUTES = (("nlls<multiexp_nlls,2>", "plugin", "auto"), ("nlls_wave<multiexp_nlls>", "plugin", "wave"), ("nlls<exp,2>", "exp", "auto"))
results = []
L = hiplib.lib()
nl = vbabi.FvbNlls.defaults(False)


def problems(V):
    ref, y = cases.exp_problem(V, T, 1, DT, seed=1)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_nlls", num_exps=1, dt=DT,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1))
    for h in (ref, dev):
        h.set_post_mean([0.0, 0.0])  # (the start of the built-in models)
        h.cfg.data_f64 = 0
        # fabber_nlls_run_device takes DEVICE pointers: the one array these configurations point to goes up
        # (the wave minimiser reads it for masked timepoints; a host pointer there is an illegal access)
        h.keep["phi_index_device"] = torch.from_numpy(h.keep["phi_index"]).to("cuda:0")
        h.cfg.phi_index = h.keep["phi_index_device"].data_ptr()
        assert not h.cfg.design and not h.cfg.model_consts and not h.cfg.params_ext
    return {"plugin": dev, "exp": ref}, y


for V in (65536, 262144):
    holders, y = problems(V)
    series = torch.from_numpy(y).to("cuda:0")
    mvn = torch.zeros((vbabi.mvn_rows(2), V), dtype=torch.float64, device="cuda:0")
    out = vbabi.FvbOutputs()
    out.mvn = mvn.data_ptr()

    def run(which):
        rc = L.fabber_nlls_run_device(C.byref(holders[which].cfg), C.byref(nl), series.data_ptr(), C.byref(out), None, T)
        assert rc == 0, L.fabber_vb_last_error().decode()

    means = {}
    for name, which, variant in ROUTES:
        hiplib.set_variant(variant)
        assert hiplib.nlls_kernel_name(holders[which]) == name, (hiplib.nlls_kernel_name(holders[which]), name)
        print("warm-up %7d voxels  %s" % (V, name), flush=True)
        run(which)  # (code object)
        torch.cuda.synchronize()
        means[name] = mvn[3:5].mean(dim=1).cpu().numpy()
    ms = {name: [] for name, _, _ in ROUTES}
    for _ in range(args.rounds):
        for name, which, variant in ROUTES:
            hiplib.set_variant(variant)
            reps = 3 if name.startswith("nlls_wave") else 10  # (each window: tens of milliseconds and more)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run(which)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / reps)
    hiplib.set_variant("auto")
    kernel = {}
    for name in ms:
        med = kernel[name] = float(np.median(ms[name]))
        results.append(dict(what="kernel", voxels=V, route=name, ms_median=med, ms_min=min(ms[name]), ms_max=max(ms[name]), voxels_per_s=V / med * 1e3))
        print("kernel  %7d voxels  %-26s %9.3f ms (range %.3f .. %.3f)  %12.0f voxels/s  mean (log amp, log r) %s"
              % (V, name, med, min(ms[name]), max(ms[name]), V / med * 1e3, np.round(means[name], 5)), flush=True)
    del series, mvn

    shape = (64, 64, V // 4096)
    data = np.ascontiguousarray(y.T.reshape(shape + (T,)))
    call = {}
    for rep in (1, 2):
        for name, extra, expect in (("nlls<multiexp_nlls,2>", {}, "kernel nlls<multiexp_nlls,2>"), ("host route", {"host-model": True}, "evaluated on the host")):
            opts = dict({"model": "multiexp_nlls", "num-exps": 1, "dt": DT, "noise": "white", "method": "nlls", "save-mean": True}, **extra)
            t0 = time.perf_counter()
            res = fabber.run(data, opts, model_libs=[library])
            dt = call[name] = time.perf_counter() - t0
            assert expect in res["log"], name
            results.append(dict(what="fabber.run", voxels=V, route=name, run=rep, seconds=dt, voxels_per_s=V / dt))
            print("call %d  %7d voxels  %-26s %9.3f s   %12.0f voxels/s  mean amp %.4f" % (rep, V, name, dt, V / dt, res["mean_amp1"].mean()), flush=True)
    ratios = dict(what="ratios", voxels=V, library_lane_over_builtin_lane=kernel["nlls<exp,2>"] / kernel["nlls<multiexp_nlls,2>"],
                  library_lane_over_host_route=call["host route"] / call["nlls<multiexp_nlls,2>"])
    results.append(ratios)
    print("rates %7d voxels  library lane / built-in lane (kernel) %.3f   library device route / host route (whole call) %.2f"
          % (V, ratios["library_lane_over_builtin_lane"], ratios["library_lane_over_host_route"]), flush=True)

if args.json:
    with open(args.json, "w") as fh:
        json.dump(results, fh, indent=1)
