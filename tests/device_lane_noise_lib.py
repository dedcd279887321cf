"""Builds the test model library whose device bodies bring the lane kernels of AR(1) noise and of noise patterns
(tests/plugins/fwdmodel_lane_noise_models.hip: multiexp_lanenz, invrec_lanenz) with the builder of the other test
libraries, and says how long each part took to compile."""
import device_model_lib

LIBRARY = "libfabber_models_lane_noise.so"
PARTS = (1, 2, 3, 4, 5)
ENTRIES = {("multiexp_lanenz", 2), ("multiexp_lanenz", 4), ("invrec_lanenz", 3)}


def build_lane_noise_library():
    """bodies with a FABBER_DEVICE_LANE_NOISE_MODEL line each (multiexp_lanenz P = 4: AR(1) only)"""
    first = LIBRARY not in device_model_lib.seconds
    path = device_model_lib.build("fwdmodel_lane_noise_models.hip", PARTS, LIBRARY)
    if first:
        print("lane noise model library: compile seconds per part %s"
              % {k: round(v, 1) for k, v in sorted(device_model_lib.seconds[LIBRARY].items())})
    return path
