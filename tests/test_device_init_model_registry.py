"""The initial-posterior kernel for the device bodies of model libraries, the part that needs no GPU: the SDK header
(include/fabber_device_init_model.h) and the test library (tests/plugins/fwdmodel_init_models.hip) compile for gfx950,
loading the library registers its names, the engine names the library's kernel exactly where a run without init_mvn would
go through it (fabber_vb_init_posterior_kernel_name), and the registry refuses what it must
(fabber_vb_register_device_init_model: codes -90 to -94)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import device_init_lib
import device_model_lib
from fabber_core_amd import hiplib, vbabi

pytestmark = [pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]


@pytest.fixture(scope="module")
def library():
    path = device_init_lib.build_init_library()
    print("init model library: compile seconds per part %s"
          % {k: round(v, 1) for k, v in sorted(device_model_lib.seconds[device_init_lib.LIBRARY].items())})
    hiplib.load_model_library(path)
    return path


@vbabi.FvbDeviceInitModel.LAUNCH_FN
def _never_launched(cfg, data, init_mvn, stream, err, err_len):
    return -1


def config_size():
    """sizeof(fvb_config) as the engine was compiled with it: its refusal of a descriptor with another size states it"""
    d = vbabi.FvbDeviceInitModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, _never_launched)
    assert hiplib.lib().fabber_vb_register_device_init_model(C.byref(d)) == -92
    m = re.search(r"fvb_config 0 against (\d+) bytes\)", hiplib.lib().fabber_vb_last_error().decode())
    return int(m.group(1))


def descriptor(name, abi=vbabi.FVB_ABI_VERSION, config=None):
    d = vbabi.FvbDeviceInitModel()
    d.name = name.encode()
    d.abi_version = abi
    d.config_size = config_size() if config is None else config
    d.launch = _never_launched
    return d


INVREC_PARAMS = [dict(name="M0", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
                 dict(name="T1", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG),
                 dict(name="a", prior=(0.8, 4.0), post=(0.8, 1.0), prior_type="N", transform=vbabi.TRANSFORM_FRACTIONAL)]


def invrec_config(name="invrec_init", V=70, T=12, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, constants=np.linspace(0.1, 3.0, T), params=INVREC_PARAMS, **kw)


def multiexp_config(num_exps, name="multiexp_init", V=70, T=21, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, num_exps=num_exps, dt=0.04,
                              params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **kw)


def test_the_engine_struct_is_the_python_one():
    """(the descriptor's size is that of the struct the launcher receives)"""
    assert config_size() == C.sizeof(vbabi.FvbConfig)


def test_library_compiles_and_registers_its_names(library):
    assert os.path.exists(library)
    assert {"multiexp_init", "invrec_init", "multiexp_noinit"} <= set(hiplib.device_models())
    assert {"multiexp_init", "invrec_init"} <= set(hiplib.device_init_models())
    assert "multiexp_noinit" not in hiplib.device_init_models()
    assert ("multiexp_init", 2) in hiplib.device_lane_models() and ("multiexp_init", 2) in hiplib.device_lane_noise_models()
    assert ("multiexp_init", 2) in hiplib.device_spatial_models()
    # count and name, as the C functions answer them
    L = hiplib.lib()
    n = L.fabber_vb_device_init_model_count()
    assert n == len(hiplib.device_init_models()) >= 2
    assert L.fabber_vb_device_init_model_name(n) is None and L.fabber_vb_device_init_model_name(-1) is None
    assert L.fabber_vb_device_init_model_name(0).decode() == hiplib.device_init_models()[0]


def test_kernel_name_is_the_library_kernel_where_a_run_without_init_mvn_goes_through_it(library):
    assert hiplib.init_posterior_kernel_name(invrec_config()) == "init<invrec_init>"
    assert hiplib.init_posterior_kernel_name(multiexp_config(1)) == "init<multiexp_init>"
    assert hiplib.init_posterior_kernel_name(multiexp_config(17)) == "init<multiexp_init>"  # (P = 34: the parameter table)
    assert hiplib.init_posterior_kernel_name(multiexp_config(1, noise=vbabi.NOISE_AR1, num_echoes=1)) == "init<multiexp_init>"
    # a body without an entry: a run without init_mvn is refused, there is no kernel
    assert hiplib.init_posterior_kernel_name(multiexp_config(1, name="multiexp_noinit")) == ""
    # the built-in models initialise themselves inside their fit kernels
    assert hiplib.init_posterior_kernel_name(vbabi.build_config(vbabi.MODEL_EXP, 70, 21, num_exps=1, dt=0.04)) == ""
    # a given init_mvn always wins: the entry is not consulted
    given = invrec_config(init_mvn=np.zeros((vbabi.mvn_rows(4), 70)))
    assert hiplib.init_posterior_kernel_name(given) == ""
    # a configuration the entry points refuse outright has no kernel
    bad = invrec_config()
    bad.cfg.n_times = 0
    assert hiplib.init_posterior_kernel_name(bad) == ""


def test_registry_refuses_bad_descriptors_abi_sizes_and_duplicates(library):
    L = hiplib.lib()
    assert L.fabber_vb_register_device_init_model(None) == -90
    no_launcher = descriptor("no_launcher")
    no_launcher.launch = vbabi.FvbDeviceInitModel.LAUNCH_FN()
    assert L.fabber_vb_register_device_init_model(C.byref(no_launcher)) == -90
    no_name = descriptor("x")
    no_name.name = None
    assert L.fabber_vb_register_device_init_model(C.byref(no_name)) == -90
    assert L.fabber_vb_unregister_device_init_model(None) == -90
    with pytest.raises(hiplib.HipEngineError, match="-90.*the name is longer than %d characters" % (vbabi.FVB_DEVICE_MODEL_NAME_MAX - 1)):
        hiplib.register_device_init_model(descriptor("n" * vbabi.FVB_DEVICE_MODEL_NAME_MAX))
    with pytest.raises(hiplib.HipEngineError, match="-91.*built for ABI version %d" % (vbabi.FVB_ABI_VERSION - 1)):
        hiplib.register_device_init_model(descriptor("other_abi", abi=vbabi.FVB_ABI_VERSION - 1))
    size = config_size()
    with pytest.raises(hiplib.HipEngineError, match="-92.*struct size mismatch \\(fvb_config %d against %d bytes\\)" % (size + 8, size)):
        hiplib.register_device_init_model(descriptor("other_config", config=size + 8))
    with pytest.raises(hiplib.HipEngineError, match="-93.*'invrec_init' is already registered"):
        hiplib.register_device_init_model(descriptor("invrec_init"))
    with pytest.raises(hiplib.HipEngineError, match="-94.*'never_there'"):
        hiplib.unregister_device_init_model("never_there")
    assert not {"no_launcher", "x", "other_abi", "other_config", "n" * vbabi.FVB_DEVICE_MODEL_NAME_MAX} & set(hiplib.device_init_models())


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
    h = invrec_config(name="orphan_init")
    assert hiplib.init_posterior_kernel_name(h) == ""
    d = descriptor("orphan_init")
    hiplib.register_device_init_model(d)
    try:
        assert "orphan_init" in hiplib.device_init_models()
        assert hiplib.init_posterior_kernel_name(h) == ""  # (an entry without a wave body of its name is never used)
        w, keep = _wave_body("orphan_init")
        hiplib.register_device_model(w)
        try:
            assert hiplib.init_posterior_kernel_name(h) == "init<orphan_init>"
            hiplib.unregister_device_init_model("orphan_init")
            assert "orphan_init" not in hiplib.device_init_models() and "invrec_init" in hiplib.device_init_models()
            assert hiplib.init_posterior_kernel_name(h) == ""
            with pytest.raises(hiplib.HipEngineError, match="-94.*'orphan_init'"):
                hiplib.unregister_device_init_model("orphan_init")
        finally:
            hiplib.unregister_device_model("orphan_init")
    finally:
        if "orphan_init" in hiplib.device_init_models():
            hiplib.unregister_device_init_model("orphan_init")
    assert hiplib.init_posterior_kernel_name(invrec_config()) == "init<invrec_init>"


def test_the_refusals_of_the_entry_point_need_no_device(library):
    """-95 comes before anything touches a device: a body without an entry (with the macro's name in the message) and a
    built-in model"""
    L = hiplib.lib()
    y = np.zeros((21, 70), dtype=np.float32)
    img = np.zeros((vbabi.mvn_rows(3), 70))
    h = multiexp_config(1, name="multiexp_noinit")
    assert L.fabber_vb_init_posterior_host(C.byref(h.cfg), y.ctypes.data, img.ctypes.data, 0) == -95
    assert re.search(r"'multiexp_noinit'.*FABBER_DEVICE_INIT_MODEL", L.fabber_vb_last_error().decode())
    b = vbabi.build_config(vbabi.MODEL_EXP, 70, 21, num_exps=1, dt=0.04)
    assert L.fabber_vb_init_posterior_host(C.byref(b.cfg), y.ctypes.data, img.ctypes.data, 0) == -95
    assert "built-in model" in L.fabber_vb_last_error().decode()
