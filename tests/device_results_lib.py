"""Builds the test model library whose device bodies bring the result-image kernel
(tests/plugins/fwdmodel_results_models.hip: multiexp_res, invrec_res) with the builder of the other test libraries."""
import device_model_lib

LIBRARY = "libfabber_models_results.so"
PARTS = (1, 2, 3, 4)


def build_results_library():
    """bodies with a results entry each (multiexp_res: also lane kernels for P = 2)"""
    return device_model_lib.build("fwdmodel_results_models.hip", PARTS, LIBRARY)
