"""The result-image kernel (model fit and residuals) for the device bodies of model libraries, the part that needs no
GPU: the SDK header (include/fabber_device_results_model.h) and the test library
(tests/plugins/fwdmodel_results_models.hip) compile for gfx950, loading the library registers its names, the engine names
the library's kernel exactly where a fit request would go through it (fabber_vb_postproc_kernel_name), and the registry
refuses what it must (fabber_vb_register_device_results_model)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import device_model_lib
import device_results_lib
from fabber_core_amd import hiplib, vbabi

pytestmark = [pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]


@pytest.fixture(scope="module")
def library():
    path = device_results_lib.build_results_library()
    print("results model library: compile seconds per part %s"
          % {k: round(v, 1) for k, v in sorted(device_model_lib.seconds[device_results_lib.LIBRARY].items())})
    hiplib.load_model_library(path)
    return path


@vbabi.FvbDeviceResultsModel.LAUNCH_FN
def _never_launched(cfg, data, mvn, pp, n_noise, stream, err, err_len):
    return -1


def struct_sizes():
    """sizeof(fvb_config) and sizeof(fvb_postproc) as the engine was compiled with them: its refusal of a descriptor with
    other sizes states both"""
    d = vbabi.FvbDeviceResultsModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 0, _never_launched)
    assert hiplib.lib().fabber_vb_register_device_results_model(C.byref(d)) == -82
    m = re.search(r"fvb_config 0 against (\d+) bytes, fvb_postproc 0 against (\d+)\)", hiplib.lib().fabber_vb_last_error().decode())
    return int(m.group(1)), int(m.group(2))


def descriptor(name, abi=vbabi.FVB_ABI_VERSION, config=None, postproc=None):
    sizes = struct_sizes()
    d = vbabi.FvbDeviceResultsModel()
    d.name = name.encode()
    d.abi_version = abi
    d.config_size = sizes[0] if config is None else config
    d.postproc_size = sizes[1] if postproc is None else postproc
    d.launch = _never_launched
    return d


INVREC_PARAMS = [dict(name="M0", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
                 dict(name="T1", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG),
                 dict(name="a", prior=(0.8, 4.0), post=(0.8, 1.0), prior_type="N", transform=vbabi.TRANSFORM_FRACTIONAL)]


def invrec_config(name="invrec_res", V=210, T=12, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, constants=np.linspace(0.1, 3.0, T), params=INVREC_PARAMS, **kw)


def multiexp_config(num_exps, name="multiexp_res", V=210, T=21, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, num_exps=num_exps, dt=0.04,
                              params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **kw)


def test_the_engine_structs_are_the_python_ones():
    """(the descriptor's sizes are those of the two structs the launcher receives)"""
    assert struct_sizes() == (C.sizeof(vbabi.FvbConfig), C.sizeof(vbabi.FvbPostproc))


def test_library_compiles_and_registers_both_names(library):
    assert os.path.exists(library)
    assert {"multiexp_res", "invrec_res"} <= set(hiplib.device_models())
    assert {"multiexp_res", "invrec_res"} <= set(hiplib.device_results_models())
    assert ("multiexp_res", 2) in hiplib.device_lane_models()


def test_kernel_name_is_the_library_kernel_where_a_fit_request_goes_through_it(library):
    assert hiplib.postproc_kernel_name(invrec_config()) == "postproc<invrec_res>"
    assert hiplib.postproc_kernel_name(multiexp_config(1)) == "postproc<multiexp_res>"
    assert hiplib.postproc_kernel_name(multiexp_config(17)) == "postproc<multiexp_res>"  # (P = 34: the parameter table)
    # the built-in models: the engine's own kernel
    assert hiplib.postproc_kernel_name(vbabi.build_config(vbabi.MODEL_EXP, 210, 21, num_exps=1, dt=0.04)) == "postproc"
    # a configuration the entry point refuses outright has no kernel
    bad = invrec_config()
    bad.cfg.n_times = 0
    assert hiplib.postproc_kernel_name(bad) == ""


def test_a_wave_body_without_a_results_entry_has_no_kernel(library):
    """the library of tests/plugins/fwdmodel_device_models.hip registers wave bodies only"""
    hiplib.load_model_library(device_model_lib.build_library())
    assert "multiexp_dev" in hiplib.device_models() and "multiexp_dev" not in hiplib.device_results_models()
    assert hiplib.postproc_kernel_name(multiexp_config(1, name="multiexp_dev")) == ""


def test_registry_refuses_bad_descriptors_abi_sizes_and_duplicates(library):
    L = hiplib.lib()
    assert L.fabber_vb_register_device_results_model(None) == -80
    no_launcher = descriptor("no_launcher")
    no_launcher.launch = vbabi.FvbDeviceResultsModel.LAUNCH_FN()
    assert L.fabber_vb_register_device_results_model(C.byref(no_launcher)) == -80
    with pytest.raises(hiplib.HipEngineError, match="-80.*the name is longer than %d characters" % (vbabi.FVB_DEVICE_MODEL_NAME_MAX - 1)):
        hiplib.register_device_results_model(descriptor("n" * vbabi.FVB_DEVICE_MODEL_NAME_MAX))
    with pytest.raises(hiplib.HipEngineError, match="-81.*built for ABI version %d" % (vbabi.FVB_ABI_VERSION - 1)):
        hiplib.register_device_results_model(descriptor("other_abi", abi=vbabi.FVB_ABI_VERSION - 1))
    config, postproc = struct_sizes()
    with pytest.raises(hiplib.HipEngineError, match="-82.*struct size mismatch \\(fvb_config %d against %d bytes, fvb_postproc %d against %d\\)"
                       % (config + 8, config, postproc, postproc)):
        hiplib.register_device_results_model(descriptor("other_config", config=config + 8))
    with pytest.raises(hiplib.HipEngineError, match="-82.*struct size mismatch \\(fvb_config %d against %d bytes, fvb_postproc %d against %d\\)"
                       % (config, config, postproc + 8, postproc)):
        hiplib.register_device_results_model(descriptor("other_postproc", postproc=postproc + 8))
    with pytest.raises(hiplib.HipEngineError, match="-83.*'invrec_res' is already registered"):
        hiplib.register_device_results_model(descriptor("invrec_res"))
    with pytest.raises(hiplib.HipEngineError, match="-84.*'never_there'"):
        hiplib.unregister_device_results_model("never_there")
    assert not {"no_launcher", "other_abi", "other_config", "other_postproc", "n" * vbabi.FVB_DEVICE_MODEL_NAME_MAX} & set(hiplib.device_results_models())


def _wave_body(name):
    """a wave body of that name, never launched (the sizes as the engine's refusal of a probe states them)"""
    @vbabi.FvbDeviceModel.LAUNCH_FN
    def never(kernel_args, stream, err, err_len):
        return -1
    probe = vbabi.FvbDeviceModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 0, never)
    assert hiplib.lib().fabber_vb_register_device_model(C.byref(probe)) == -72
    sizes = re.search(r"KernelArgs 0 against (\d+) bytes, WaveLayout 0 against (\d+)\)", hiplib.lib().fabber_vb_last_error().decode())
    return vbabi.FvbDeviceModel(name.encode(), vbabi.FVB_ABI_VERSION, int(sizes.group(1)), int(sizes.group(2)), never), never


def test_an_entry_needs_a_wave_body_and_unregistering_returns_the_configuration_to_no_kernel(library):
    # (a configuration that names an unregistered body is refused by the argument checks: no kernel)
    h = invrec_config(name="orphan_res")
    assert hiplib.postproc_kernel_name(h) == ""
    d = descriptor("orphan_res")
    hiplib.register_device_results_model(d)
    try:
        assert "orphan_res" in hiplib.device_results_models()
        assert hiplib.postproc_kernel_name(h) == ""  # (an entry without a wave body of its name is never used)
        w, keep = _wave_body("orphan_res")
        hiplib.register_device_model(w)
        try:
            assert hiplib.postproc_kernel_name(h) == "postproc<orphan_res>"
            hiplib.unregister_device_results_model("orphan_res")
            assert "orphan_res" not in hiplib.device_results_models() and "invrec_res" in hiplib.device_results_models()
            assert hiplib.postproc_kernel_name(h) == ""
            with pytest.raises(hiplib.HipEngineError, match="-84.*'orphan_res'"):
                hiplib.unregister_device_results_model("orphan_res")
        finally:
            hiplib.unregister_device_model("orphan_res")
    finally:
        if "orphan_res" in hiplib.device_results_models():
            hiplib.unregister_device_results_model("orphan_res")
    assert hiplib.postproc_kernel_name(invrec_config()) == "postproc<invrec_res>"
