"""Builds the test model library whose device bodies bring a sweep of their own (tests/plugins/fwdmodel_sweep_models.hip:
multiexp_sw, multiexp_swchk) with the builder of the other test libraries, and says how long each part took to compile."""
import device_model_lib

LIBRARY = "libfabber_models_sweep.so"
PARTS = (1, 2, 3, 4, 5, 6, 7, 8, 9)
LANE_ENTRIES = {("multiexp_sw", 2), ("multiexp_sw", 4), ("multiexp_swchk", 2)}
LANE_NOISE_ENTRIES = {("multiexp_sw", 2), ("multiexp_swchk", 2)}


def build_sweep_library():
    """bodies with `template <int P> struct Sweep` and a macro line of every lane family"""
    first = LIBRARY not in device_model_lib.seconds
    path = device_model_lib.build("fwdmodel_sweep_models.hip", PARTS, LIBRARY)
    if first:
        print("sweep model library: compile seconds per part %s"
              % {k: round(v, 1) for k, v in sorted(device_model_lib.seconds[LIBRARY].items())})
    return path
