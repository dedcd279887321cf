"""Builds the test model library whose device bodies bring the initial-posterior kernel
(tests/plugins/fwdmodel_init_models.hip: multiexp_init, invrec_init, and multiexp_noinit without an entry) with the builder
of the other test libraries."""
import device_model_lib

LIBRARY = "libfabber_models_init.so"
PARTS = (1, 2, 3, 4, 5, 6, 7)  # (the last one holds the init lines)


def build_init_library():
    """bodies with an init entry each (multiexp_init: also lane kernels under the three noise models and spatial kernels
    for P = 2), and a wave body without one"""
    return device_model_lib.build("fwdmodel_init_models.hip", PARTS, LIBRARY)
