"""NLLS minimisers for the device bodies of model libraries, the part that needs no GPU: the SDK header
(include/fabber_device_nlls_model.h) and the test library (tests/plugins/fwdmodel_nlls_models.hip) compile for gfx950,
loading the library registers its (name, parameter count) entries, the engine names the minimiser a configuration would
run on (fabber_nlls_kernel_name), and the registry refuses what it must (fabber_vb_register_device_nlls_model)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import device_model_lib
from fabber_core_amd import hiplib, vbabi

pytestmark = [pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]


@pytest.fixture(scope="module")
def library():
    path = device_model_lib.build_nlls_library()
    print("NLLS model library: compile seconds per part %s" % {k: round(v, 1) for k, v in sorted(device_model_lib.seconds["libfabber_models_nlls.so"].items())})
    hiplib.load_model_library(path)
    return path


@vbabi.FvbDeviceNllsModel.LAUNCH_FN
def _never_launched(nlls_args, stream, err, err_len):
    return -1


@vbabi.FvbDeviceModel.LAUNCH_FN
def _never_launched_wave(kernel_args, stream, err, err_len):
    return -1


def struct_sizes():
    """sizeof(fvb::NllsArgs), sizeof(fvb::WaveLayout) as the engine was compiled with them: its refusal of a descriptor
    with other sizes states both"""
    d = vbabi.FvbDeviceNllsModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 0, 3, _never_launched)
    assert hiplib.lib().fabber_vb_register_device_nlls_model(C.byref(d)) == -72
    m = re.search(r"NllsArgs 0 against (\d+) bytes, WaveLayout 0 against (\d+)\)", hiplib.lib().fabber_vb_last_error().decode())
    return int(m.group(1)), int(m.group(2))


def descriptor(name, n_params=3, abi=vbabi.FVB_ABI_VERSION, sizes=None):
    d = vbabi.FvbDeviceNllsModel()
    d.name = name.encode() if name is not None else None
    d.abi_version = abi
    d.nlls_args_size, d.wave_layout_size = struct_sizes() if sizes is None else sizes
    d.n_params = n_params
    d.launch = _never_launched
    return d


def wave_body(name):
    """a wave VB body of that name (fabber_vb_register_device_model), never launched"""
    d = vbabi.FvbDeviceModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 0, _never_launched_wave)
    assert hiplib.lib().fabber_vb_register_device_model(C.byref(d)) == -72
    sizes = re.search(r"KernelArgs 0 against (\d+) bytes, WaveLayout 0 against (\d+)\)", hiplib.lib().fabber_vb_last_error().decode())
    return vbabi.FvbDeviceModel(name.encode(), vbabi.FVB_ABI_VERSION, int(sizes.group(1)), int(sizes.group(2)), _never_launched_wave)


INVREC_PARAMS = [dict(name="M0", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
                 dict(name="T1", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG),
                 dict(name="a", prior=(0.8, 4.0), post=(0.8, 1.0), prior_type="N", transform=vbabi.TRANSFORM_FRACTIONAL)]


def invrec_config(name="invrec_nlls", V=1 << 20, T=12):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, constants=np.linspace(0.1, 3.0, T), params=INVREC_PARAMS)


def multiexp_config(num_exps, V=1 << 20, T=50):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_nlls", num_exps=num_exps, dt=0.04,
                              params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps))


def test_library_compiles_and_registers_its_entries(library):
    assert os.path.exists(library)
    assert {"multiexp_nlls", "invrec_nlls"} <= set(hiplib.device_models())
    assert {("multiexp_nlls", 0), ("multiexp_nlls", 2), ("multiexp_nlls", 4), ("invrec_nlls", 0), ("invrec_nlls", 3)} <= set(hiplib.device_nlls_models())


def test_kernel_name_follows_the_size_rule_of_the_built_in_models(library):
    assert hiplib.nlls_kernel_name(invrec_config()) == "nlls<invrec_nlls,3>"
    assert hiplib.nlls_kernel_name(invrec_config(V=4096)) == "nlls<invrec_nlls,3>"
    assert hiplib.nlls_kernel_name(invrec_config(V=4095)) == "nlls_wave<invrec_nlls>"
    assert hiplib.nlls_kernel_name(invrec_config(V=512)) == "nlls_wave<invrec_nlls>"
    assert hiplib.nlls_kernel_name(multiexp_config(1)) == "nlls<multiexp_nlls,2>"
    assert hiplib.nlls_kernel_name(multiexp_config(2)) == "nlls<multiexp_nlls,4>"
    assert hiplib.nlls_kernel_name(multiexp_config(3)) == "nlls_wave<multiexp_nlls>"  # (P = 6: no entry in this library)
    # the built-in models keep their names
    assert hiplib.nlls_kernel_name(vbabi.build_config(vbabi.MODEL_EXP, 1 << 20, 50, num_exps=1, dt=0.04)) == "nlls<exp,2>"
    assert hiplib.nlls_kernel_name(vbabi.build_config(vbabi.MODEL_EXP, 512, 50, num_exps=1, dt=0.04)) == "nlls_wave"
    assert hiplib.nlls_kernel_name(vbabi.build_config(vbabi.MODEL_POLY, 1 << 20, 10, degree=7)) == "nlls_wave"  # (P = 8: no lane minimiser)


def test_variant_overrides_the_size_rule(library):
    hiplib.set_variant("lane")
    try:
        assert hiplib.nlls_kernel_name(invrec_config(V=512)) == "nlls<invrec_nlls,3>"
        assert hiplib.nlls_kernel_name(multiexp_config(3, V=512)) == "nlls_wave<multiexp_nlls>"
        assert hiplib.nlls_kernel_name(vbabi.build_config(vbabi.MODEL_EXP, 512, 50, num_exps=1, dt=0.04)) == "nlls<exp,2>"
    finally:
        hiplib.set_variant("auto")
    hiplib.set_variant("wave")
    try:
        assert hiplib.nlls_kernel_name(invrec_config()) == "nlls_wave<invrec_nlls>"
        assert hiplib.nlls_kernel_name(vbabi.build_config(vbabi.MODEL_EXP, 1 << 20, 50, num_exps=1, dt=0.04)) == "nlls_wave"
    finally:
        hiplib.set_variant("auto")
    assert hiplib.nlls_kernel_name(invrec_config()) == "nlls<invrec_nlls,3>"


def test_a_body_without_nlls_entries_has_no_kernel(library):
    """the library of tests/plugins/fwdmodel_device_models.hip registers wave VB bodies only: method=nlls stays where it was"""
    hiplib.load_model_library(device_model_lib.build_library())
    assert "invrec" in hiplib.device_models() and "invrec" not in [n for n, _ in hiplib.device_nlls_models()]
    assert hiplib.nlls_kernel_name(invrec_config(name="invrec")) == ""
    assert "device body" in hiplib.lib().fabber_vb_last_error().decode()
    assert hiplib.nlls_kernel_name(invrec_config(name="no_such_model")) == ""
    hostjac = invrec_config(V=64)
    hostjac.cfg.model = vbabi.MODEL_HOSTJAC  # (a model that exists only as host code)
    assert hiplib.nlls_kernel_name(hostjac) == ""


def test_registry_refuses_wrong_abi_sizes_counts_and_duplicates(library):
    nlls_args, wave_layout = struct_sizes()
    with pytest.raises(hiplib.HipEngineError, match="-71.*built for ABI version %d" % (vbabi.FVB_ABI_VERSION - 1)):
        hiplib.register_device_nlls_model(descriptor("other_abi", abi=vbabi.FVB_ABI_VERSION - 1))
    with pytest.raises(hiplib.HipEngineError, match="-72.*NllsArgs %d against %d bytes, WaveLayout %d against %d" % (nlls_args + 8, nlls_args, wave_layout, wave_layout)):
        hiplib.register_device_nlls_model(descriptor("other_args", sizes=(nlls_args + 8, wave_layout)))
    with pytest.raises(hiplib.HipEngineError, match="-72.*WaveLayout %d against %d" % (wave_layout + 4, wave_layout)):
        hiplib.register_device_nlls_model(descriptor("other_layout", n_params=0, sizes=(nlls_args, wave_layout + 4)))
    for n in (-1, 7):
        with pytest.raises(hiplib.HipEngineError, match="-70.*%d parameters .*1 to 6" % n):
            hiplib.register_device_nlls_model(descriptor("other_count", n_params=n))
    with pytest.raises(hiplib.HipEngineError, match="-70.*name or launcher is NULL"):
        hiplib.register_device_nlls_model(descriptor(None))
    with pytest.raises(hiplib.HipEngineError, match="-70.*longer than %d characters" % (vbabi.FVB_DEVICE_MODEL_NAME_MAX - 1)):
        hiplib.register_device_nlls_model(descriptor("n" * vbabi.FVB_DEVICE_MODEL_NAME_MAX))
    with pytest.raises(hiplib.HipEngineError, match="-73.*'invrec_nlls' with 3 parameters is already registered"):
        hiplib.register_device_nlls_model(descriptor("invrec_nlls", n_params=3))
    with pytest.raises(hiplib.HipEngineError, match="-73.*wave NLLS minimiser.*'invrec_nlls' is already registered"):
        hiplib.register_device_nlls_model(descriptor("invrec_nlls", n_params=0))
    assert hiplib.lib().fabber_vb_register_device_nlls_model(None) == -70
    with pytest.raises(hiplib.HipEngineError, match="-74.*'invrec_nlls' with 5 parameters is not registered"):
        hiplib.unregister_device_nlls_model("invrec_nlls", 5)
    assert not {"other_abi", "other_args", "other_layout", "other_count"} & {n for n, _ in hiplib.device_nlls_models()}


def test_a_lane_entry_counts_only_next_to_the_wave_minimiser_and_unregistering_restores_the_answers(library):
    body = wave_body("orphan_nlls")
    lane, wave = descriptor("orphan_nlls", n_params=3), descriptor("orphan_nlls", n_params=0)
    hiplib.register_device_nlls_model(lane)
    try:
        # neither a body nor the wave minimiser; then the body alone
        assert hiplib.nlls_kernel_name(invrec_config(name="orphan_nlls")) == ""
        assert "no device model 'orphan_nlls' is registered" in hiplib.lib().fabber_vb_last_error().decode()
        hiplib.register_device_model(body)
        try:
            assert hiplib.nlls_kernel_name(invrec_config(name="orphan_nlls")) == ""
            assert "device body" in hiplib.lib().fabber_vb_last_error().decode()
            hiplib.register_device_nlls_model(wave)
            try:
                assert ("orphan_nlls", 0) in hiplib.device_nlls_models() and ("orphan_nlls", 3) in hiplib.device_nlls_models()
                assert hiplib.nlls_kernel_name(invrec_config(name="orphan_nlls")) == "nlls<orphan_nlls,3>"
                assert hiplib.nlls_kernel_name(invrec_config(name="orphan_nlls", V=512)) == "nlls_wave<orphan_nlls>"
            finally:
                hiplib.unregister_device_nlls_model("orphan_nlls", 0)
            assert hiplib.nlls_kernel_name(invrec_config(name="orphan_nlls")) == ""
        finally:
            hiplib.unregister_device_model("orphan_nlls")
    finally:
        hiplib.unregister_device_nlls_model("orphan_nlls", 3)
    assert not [e for e in hiplib.device_nlls_models() if e[0] == "orphan_nlls"]
    assert hiplib.nlls_kernel_name(invrec_config()) == "nlls<invrec_nlls,3>"
