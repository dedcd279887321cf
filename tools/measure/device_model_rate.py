"""The problem of hostmodel_rate.py through both routes of a model library's model with a device body (multiexp_dev
of tests/plugins/fwdmodel_device_models.hip): the device route (the library's wave-per-voxel kernels) and the host-model
route (2P + 1 EvaluateModel calls per voxel and re-centre, 16 host threads), same build, same process, in this order.
Each route is run twice; the second run (warm device, library loaded) is the one to quote."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import device_model_lib
from fabber_core_amd import fabber

library = device_model_lib.build_library()
rng = np.random.default_rng(0)
shape, T = (64, 64, 16), 50
t = np.arange(T) * 0.04
data = (np.exp(-t) + rng.normal(0, 0.1, shape + (T,))).astype(np.float32)
opts = {"model": "multiexp_dev", "num-exps": 1, "dt": 0.04, "noise": "white", "method": "vb", "max-iterations": 10, "save-mean": True}
V = np.prod(shape)
for label, extra in (("device body", {}), ("host model, 16 threads", {"host-model": True, "host-model-threads": 16}),
                     ("device body", {}), ("host model, 16 threads", {"host-model": True, "host-model-threads": 16})):
    t0 = time.perf_counter()
    out = fabber.run(data, dict(opts, **extra), model_libs=[library])
    dt = time.perf_counter() - t0
    route = "wave<multiexp_dev>" if "of its library" in out["log"] else "host"
    print("%-26s %7.3f s  %9.0f voxels/s  route %-20s mean amp %.4f" % (label, dt, V / dt, route, out["mean_amp1"].mean()), flush=True)
