"""Lane against wave for a model library's device bodies under AR(1) noise and under a noise pattern: invrec_lanenz and
multiexp_lanenz (one exponential) of tests/plugins/fwdmodel_lane_noise_models.hip at 65 536 voxels, 10 iterations, through
the host entry point of the C ABI (upload and download included, as in device_model_rate.py), the route chosen with
set_variant. Every step - one model, one noise model, one route - is a process of its own under a time limit; it runs
the problem twice and reports the second run (warm device, library loaded). A step that fails or runs out of time ends the
measurement: nothing more is started on the device after it.

    python tools/measure/device_lane_noise_rate.py [--library PATH] [--json OUT]

--library: a built libfabber_models_lane_noise.so (default: built here first, about a minute and a half)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

V, ITERATIONS, STEP_SECONDS = 65536, 10, 120
MODELS = ("invrec_lanenz", "multiexp_lanenz")
NOISES = ("ar1", "pattern 12")
ROUTES = ("lane", "wave")


def problem(model, noise):
    import numpy as np
    import test_device_lane_noise_model as t
    from test_device_model import initial_mvn
    import cases
    from fabber_core_amd import vbabi
    opts = dict(max_iterations=ITERATIONS, **t.NOISES[noise])
    if model == "invrec_lanenz":
        y = t.invrec_series(V, seed=1)
        return t.invrec_problem(y, **opts), y
    ref, y = cases.exp_problem(V, 50, 1, 0.04, seed=1, **opts)
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, 50, device_model=model, num_exps=1, dt=0.04, init_mvn=initial_mvn(ref, y),
                              params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1), **opts), y


def step(library, model, noise, route):
    import numpy as np
    from fabber_core_amd import hiplib
    hiplib.load_model_library(library)
    h, y = problem(model, noise)
    hiplib.set_variant(route)
    kernel = hiplib.kernel_name(h)
    assert kernel.startswith("wave<" if route == "wave" else "lane_"), kernel
    seconds = []
    for _ in range(2):
        t0 = time.perf_counter()
        r = hiplib.run_host(h, y)
        seconds.append(time.perf_counter() - t0)
    assert np.all(r["status"] == 0), "bad voxels: %d" % int((r["status"] != 0).sum())
    print(json.dumps(dict(model=model, noise=noise, route=route, kernel=kernel, voxels=V, timepoints=int(h.cfg.n_times), iterations=ITERATIONS,
                          first_s=seconds[0], second_s=seconds[1], voxels_per_s=V / seconds[1])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", nargs=3, default=None, help="(internal) model, noise, route: run this one step in this process")
    a = ap.parse_args()
    if a.step:
        return step(a.library, *a.step)
    library = a.library
    if not library:
        import device_lane_noise_lib
        library = device_lane_noise_lib.build_lane_noise_library()
    results = []
    for model in MODELS:
        for noise in NOISES:
            for route in ROUTES:
                try:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--library", library, "--step", model, noise, route],
                                       capture_output=True, text=True, timeout=STEP_SECONDS)
                except subprocess.TimeoutExpired:
                    sys.exit("%s, %s, %s: no answer within %d s - the measurement ends here" % (model, noise, route, STEP_SECONDS))
                if p.returncode != 0:
                    sys.exit("%s, %s, %s: exit status %d - the measurement ends here\n%s" % (model, noise, route, p.returncode, p.stderr[-2000:]))
                r = json.loads(p.stdout.strip().splitlines()[-1])
                results.append(r)
                print("%-16s %-10s %-4s %-30s %7.4f s  %10.0f voxels/s" % (model, noise, route, r["kernel"], r["second_s"], r["voxels_per_s"]),
                      flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
