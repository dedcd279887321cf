"""Spatial VB of a host-evaluated model with 12 parameters (the wave-per-voxel family, csrc/vb_spatial_wave.h): a design
of 12 cosine regressors on a masked 64 x 64 x 24 volume, T = 60, priors M, M, ARD and N, g and J handed over exactly.
Prints one JSON line: ms per spatial iteration, split into the host's linearisation (the callback) and the rest (the
engine: both sweeps, the a_K updates, the means' download and the linearisations' upload). Per-iteration figures are
differences between runs of K1 and K2 iterations, so the set-up (geometry, first linearisation) cancels.
Usage: python tools/measure/spatial_wide_rate.py [--k1 2] [--k2 6] [--iterations-only N (one run, for a profiler)]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from fabber_core_amd import hiplib, vbabi  # noqa: E402


def problem(shape=(64, 64, 24), T=60, P=12, seed=0):
    rng = np.random.default_rng(seed)
    mask = rng.random(shape) < 0.85
    coords = vbabi.grid_coords(shape, mask)
    t = np.arange(T)
    X = np.cos(np.pi * np.arange(P)[None, :] * (t[:, None] + 0.5) / T)
    x, yy, z = coords
    theta = np.stack([1.0 / (k + 1) + 0.3 * np.sin(x / 5.0 + k) * np.cos(yy / 7.0) + 0.1 * np.sin(z / 3.0) for k in range(P)])
    y = (X @ theta + rng.normal(0, 0.1, (T, coords.shape[1]))).astype(np.float32)
    return coords, X, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k1", type=int, default=2)
    ap.add_argument("--k2", type=int, default=6)
    ap.add_argument("--iterations-only", type=int, default=0)
    a = ap.parse_args()
    coords, X, y = problem()
    V, (T, P) = coords.shape[1], X.shape
    types = ["M", "M", "A"] + ["N"] * (P - 3)
    sp = vbabi.SpatialHolder(coords)
    spent = {"s": 0.0, "calls": 0}
    bad = {"n": 0}

    def linearise(user, n, ids, means, lin):  # (hiplib.jacobian_callback's body, timed whole: g = X m, J = X, copied in)
        t0 = time.perf_counter()
        m = np.ctypeslib.as_array(means, (n * P,)).reshape(n, P)
        out = np.ctypeslib.as_array(lin, (n * T * (P + 1),)).reshape(n, T * (P + 1))
        out[:, :T] = m @ X.T
        out[:, T:] = np.broadcast_to(X, (n, T, P)).reshape(n, -1)
        spent["s"] += time.perf_counter() - t0
        spent["calls"] += 1
        return 0

    def run(iters):
        h = vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, max_iterations=iters,
                               param_overrides={"Parameter_%d" % (k + 1): dict(type=tp) for k, tp in enumerate(types)})
        spent["s"], spent["calls"] = 0.0, 0
        cb = hiplib.LINEARISE_FN(linearise)
        t0 = time.perf_counter()
        r = hiplib.run_spatial_hostmodel_host(h, sp, y, cb)
        wall = time.perf_counter() - t0
        # (a voxel of the mask without a neighbour has no M prior mean - the reference's 0 / 0 - and fails)
        bad["n"] = int(np.count_nonzero(r["status"]))
        assert bad["n"] < V // 1000 and np.isfinite(r["mvn"][:, r["status"] == 0]).all()
        return wall, spent["s"], spent["calls"]

    if a.iterations_only:
        run(a.iterations_only)
        return
    run(1)  # (library load, first use of the device)
    w1, h1, _ = run(a.k1)
    w2, h2, _ = run(a.k2)
    n = a.k2 - a.k1
    per_it, host = (w2 - w1) / n * 1e3, (h2 - h1) / n * 1e3
    rec = dict(workload="spatial VB, linear model, P=%d, T=%d, %s masked to %d voxels, host-evaluated (wave per voxel)"
               % (P, T, "64x64x24", V), ms_per_iteration=round(per_it, 2), host_linearisation_ms=round(host, 2),
               engine_ms=round(per_it - host, 2), bad_voxels=bad["n"], runs=dict(k1=a.k1, k2=a.k2, wall_s=[round(w1, 3), round(w2, 3)]))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
