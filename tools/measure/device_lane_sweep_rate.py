"""What a sweep supplied by a library's device body buys on the lane-per-voxel kernels, same build, same process: the
bi-exponential model (P = 4) over 100 timepoints, 10 iterations, at 65 536 and 1 048 576 voxels, with and without the free
energy, as

    lane<multiexp_sw,4>     the library body with its own sweep (tests/plugins/fwdmodel_sweep_models.hip)
    lane<multiexp_lane,4>   the same eval without one: 2 P + 1 pointwise evaluations per timepoint
                            (tests/plugins/fwdmodel_lane_models.hip) - the yardstick
    lane<exp,4>             the engine's built-in exponential model, whose recurrence multiexp_sw's sweep restates

Kernel time: DeviceProblem (series and results stay on the device), device events around the enqueued runs, after a
warm-up of every route; the routes alternate over the rounds, the median and the range of the rounds are printed, then the
two ratios (pointwise / sweep, sweep / built-in) of the medians.

    python tools/measure/device_lane_sweep_rate.py [--rounds 7] [--voxels 65536 1048576] [--json PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cases
import device_model_lib
import device_sweep_lib
from fabber_core_amd import hiplib, vbabi
from fabber_core_amd.device import DeviceProblem

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--voxels", type=int, nargs="+", default=[65536, 1048576])
ap.add_argument("--json", default=None)
args = ap.parse_args()

for path in (device_sweep_lib.build_sweep_library(), device_model_lib.build_lane_library()):
    hiplib.load_model_library(path)
T, DT, ITS, NUM = 100, 0.02, 10, 2
ROUTES = (("multiexp_sw", "the body's sweep"), ("multiexp_lane", "pointwise body"), ("exp", "built-in"))
results = []


def problems(V, need_f):
    opts = dict(max_iterations=ITS, need_f=need_f)
    ref, y = cases.exp_problem(V, T, NUM, DT, seed=1, **opts)
    mvn = hiplib.initial_mvn(ref, y)
    ref, _ = cases.exp_problem(V, T, NUM, DT, seed=1, init_mvn=mvn, **opts)
    holders = {"exp": ref}
    for model in ("multiexp_sw", "multiexp_lane"):
        holders[model] = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=model, num_exps=NUM, dt=DT, init_mvn=mvn,
                                            params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=NUM), **opts)
    return holders, y


for V in args.voxels:
    for need_f in (False, True):
        holders, y = problems(V, need_f)
        probs = {}
        for model, _ in ROUTES:
            name = "lane<%s,4%s>" % (model, ",F" if need_f else "")
            probs[name] = DeviceProblem(holders[model], y, "cuda:0")
            assert probs[name].kernel == name, (probs[name].kernel, name)
            probs[name].run()  # warm-up: code object, pool memory
            torch.cuda.synchronize()
        failed = {name: int(np.count_nonzero(p.results()["status"])) for name, p in probs.items()}
        reps = max(2, min(20, (20 * 65536) // V))  # (each window: tens of milliseconds and more)
        ms = {name: [] for name in probs}
        for _ in range(args.rounds):
            for name in probs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    probs[name].run()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / reps)
        med = {name: float(np.median(ms[name])) for name in probs}
        for (model, what), name in zip(ROUTES, probs):
            results.append(dict(what="kernel", voxels=V, timepoints=T, iterations=ITS, need_f=need_f, route=name, body=what, ms_median=med[name],
                                ms_min=min(ms[name]), ms_max=max(ms[name]), voxels_per_s=V / med[name] * 1e3, failed_voxels=failed[name]))
            print("kernel  %8d voxels  %-26s %9.3f ms (range %.3f .. %.3f)  %12.0f voxels/s  failed voxels %d  [%s]"
                  % (V, name, med[name], min(ms[name]), max(ms[name]), V / med[name] * 1e3, failed[name], what), flush=True)
        sw, pw, bi = list(probs)
        spread = max(max(ms[n]) - min(ms[n]) for n in (sw, pw))
        results.append(dict(what="ratios", voxels=V, need_f=need_f, pointwise_over_sweep=med[pw] / med[sw], sweep_over_builtin=med[sw] / med[bi],
                            sweep_minus_pointwise_ms=med[sw] - med[pw], round_to_round_range_ms=spread,
                            sweep_not_slower_than_pointwise=bool(med[sw] - med[pw] <= spread)))
        print("ratios  %8d voxels  F %-5s pointwise / sweep %.3f   sweep / built-in %.3f   (sweep - pointwise %.3f ms, round-to-round range %.3f ms)"
              % (V, need_f, med[pw] / med[sw], med[sw] / med[bi], med[sw] - med[pw], spread), flush=True)
        del probs

if args.json:
    with open(args.json, "w") as fh:
        json.dump(results, fh, indent=1)
