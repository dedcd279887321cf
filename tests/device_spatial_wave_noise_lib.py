"""Builds the test model library whose device bodies bring the wave-per-voxel spatial VB kernels under a noise pattern
(tests/plugins/fwdmodel_spatial_wave_noise_models.hip: multiexp_spwn, linear_spwn, suppconv_spwn, multiexp_spwn_both) for the
tests and the measuring tool of those kernels, with device_model_lib's build of a library from its parts."""
import device_model_lib

LIBRARY = "libfabber_models_spatial_wave_noise.so"
NAMES = ("multiexp_spwn", "linear_spwn", "suppconv_spwn", "multiexp_spwn_both")


def build_spatial_wave_noise_library():
    return device_model_lib.build("fwdmodel_spatial_wave_noise_models.hip", (1, 2, 3, 4, 5, 6), LIBRARY)
