"""Lane-per-voxel kernels for the device bodies of model libraries, the part that needs no GPU: the SDK header
(include/fabber_device_lane_model.h) and the test library (tests/plugins/fwdmodel_lane_models.hip) compile for gfx950,
loading the library registers its (name, parameter count) entries, the engine names the lane kernel exactly where it
takes that route, and the registry refuses what it must (fabber_vb_register_device_lane_model)."""
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
    path = device_model_lib.build_lane_library()
    print("lane model library: compile seconds per part %s" % {k: round(v, 1) for k, v in sorted(device_model_lib.seconds["libfabber_models_lane.so"].items())})
    hiplib.load_model_library(path)
    return path


@vbabi.FvbDeviceLaneModel.LAUNCH_FN
def _never_launched(kernel_args, feed, counting, stream, err, err_len):
    return -1


@vbabi.FvbDeviceModel.LAUNCH_FN
def _never_launched_wave(kernel_args, stream, err, err_len):
    return -1


def kernel_args_size():
    """sizeof(fvb::KernelArgs) as the engine was compiled with it: its refusal of a descriptor with another size states it"""
    d = vbabi.FvbDeviceLaneModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 3, 0, _never_launched)
    assert hiplib.lib().fabber_vb_register_device_lane_model(C.byref(d)) == -72
    return int(re.search(r"KernelArgs 0 against (\d+) bytes", hiplib.lib().fabber_vb_last_error().decode()).group(1))


def descriptor(name, n_params=3, abi=vbabi.FVB_ABI_VERSION, kernel_args=None):
    d = vbabi.FvbDeviceLaneModel()
    d.name = name.encode()
    d.abi_version = abi
    d.kernel_args_size = kernel_args_size() if kernel_args is None else kernel_args
    d.n_params = n_params
    d.save_rows = 30
    d.launch = _never_launched
    return d


INVREC_PARAMS = [dict(name="M0", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
                 dict(name="T1", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG),
                 dict(name="a", prior=(0.8, 4.0), post=(0.8, 1.0), prior_type="N", transform=vbabi.TRANSFORM_FRACTIONAL)]


def invrec_config(name="invrec_lane", V=1 << 20, T=12, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, constants=np.linspace(0.1, 3.0, T), params=INVREC_PARAMS, **kw)


def multiexp_config(num_exps, V=1 << 20, T=50, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_lane", num_exps=num_exps, dt=0.04,
                              params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **kw)


def test_library_compiles_and_registers_its_entries(library):
    assert os.path.exists(library)
    assert {"multiexp_lane", "invrec_lane"} <= set(hiplib.device_models())
    assert {("multiexp_lane", 2), ("multiexp_lane", 4), ("invrec_lane", 3)} <= set(hiplib.device_lane_models())


def test_kernel_name_is_the_lane_kernel_where_the_route_is_taken(library):
    assert hiplib.kernel_name(invrec_config()) == "lane<invrec_lane,3>"
    assert hiplib.kernel_name(invrec_config(need_f=True)) == "lane<invrec_lane,3,F>"
    assert hiplib.kernel_name(multiexp_config(1)) == "lane<multiexp_lane,2>"
    assert hiplib.kernel_name(multiexp_config(2, need_f=True)) == "lane<multiexp_lane,4,F>"
    # the size rule of the built-in models: 64 voxels of 12 timepoints x 7 evaluations = 84 < 400 would take the lane
    # kernel whatever the count; 16 timepoints and more of this model (>= 400 evaluations with T = 58) do not
    assert hiplib.kernel_name(invrec_config(V=64, T=58)) == "wave<invrec_lane>"
    assert hiplib.kernel_name(invrec_config(V=64, T=12)) == "lane<invrec_lane,3>"
    assert hiplib.kernel_name(invrec_config(V=4096, T=58)) == "lane<invrec_lane,3>"
    assert hiplib.kernel_name(invrec_config(V=4095, T=58)) == "wave<invrec_lane>"


def test_variant_overrides_the_size_rule(library):
    hiplib.set_variant("lane")
    try:
        assert hiplib.kernel_name(invrec_config(V=64, T=58)) == "lane<invrec_lane,3>"
    finally:
        hiplib.set_variant("auto")
    hiplib.set_variant("wave")
    try:
        assert hiplib.kernel_name(invrec_config()) == "wave<invrec_lane>"
    finally:
        hiplib.set_variant("auto")
    assert hiplib.kernel_name(invrec_config()) == "lane<invrec_lane,3>"


def test_everything_else_keeps_the_wave_kernels(library):
    assert hiplib.kernel_name(invrec_config(noise_pattern="12")) == "wave<invrec_lane>"
    assert hiplib.kernel_name(invrec_config(noise=vbabi.NOISE_AR1, num_echoes=1)) == "wave<invrec_lane>"
    assert hiplib.kernel_name(multiexp_config(3)) == "wave<multiexp_lane>"  # (P = 6: no entry)
    hiplib.set_variant("lane")
    try:
        assert hiplib.kernel_name(multiexp_config(3)) == "wave<multiexp_lane>"
        assert hiplib.kernel_name(invrec_config(noise_pattern="12")) == "wave<invrec_lane>"
    finally:
        hiplib.set_variant("auto")


def test_a_name_without_lane_entries_keeps_its_route(library):
    """the library of tests/plugins/fwdmodel_device_models.hip registers wave bodies only"""
    hiplib.load_model_library(device_model_lib.build_library())
    assert "invrec" in hiplib.device_models() and "invrec" not in [n for n, _ in hiplib.device_lane_models()]
    assert hiplib.kernel_name(invrec_config(name="invrec")) == "wave<invrec>"
    hiplib.set_variant("lane")
    try:
        assert hiplib.kernel_name(invrec_config(name="invrec", V=64)) == "wave<invrec>"
    finally:
        hiplib.set_variant("auto")


def test_registry_refuses_wrong_abi_size_counts_and_duplicates(library):
    with pytest.raises(hiplib.HipEngineError, match="-71.*built for ABI version %d" % (vbabi.FVB_ABI_VERSION - 1)):
        hiplib.register_device_lane_model(descriptor("other_abi", abi=vbabi.FVB_ABI_VERSION - 1))
    with pytest.raises(hiplib.HipEngineError, match="-72.*struct size mismatch"):
        hiplib.register_device_lane_model(descriptor("other_args", kernel_args=kernel_args_size() + 8))
    for n in (0, 7):
        with pytest.raises(hiplib.HipEngineError, match="-70.*%d parameters .*1 to 6" % n):
            hiplib.register_device_lane_model(descriptor("other_count", n_params=n))
    with pytest.raises(hiplib.HipEngineError, match="-73.*'invrec_lane' with 3 parameters are already registered"):
        hiplib.register_device_lane_model(descriptor("invrec_lane", n_params=3))
    assert hiplib.lib().fabber_vb_register_device_lane_model(None) == -70
    assert not {"other_abi", "other_args", "other_count"} & {n for n, _ in hiplib.device_lane_models()}


def test_register_and_unregister_an_entry(library):
    d = descriptor("invrec_lane", n_params=5)  # (another count of a registered name is an entry of its own)
    hiplib.register_device_lane_model(d)
    try:
        assert ("invrec_lane", 5) in hiplib.device_lane_models()
    finally:
        hiplib.unregister_device_lane_model("invrec_lane", 5)
    assert ("invrec_lane", 5) not in hiplib.device_lane_models() and ("invrec_lane", 3) in hiplib.device_lane_models()
    with pytest.raises(hiplib.HipEngineError, match="-74.*'invrec_lane' with 5 parameters"):
        hiplib.unregister_device_lane_model("invrec_lane", 5)


def test_a_lane_entry_without_a_wave_body_does_not_validate(library):
    d = descriptor("orphan_lane")
    hiplib.register_device_lane_model(d)
    try:
        assert hiplib.kernel_name(invrec_config(name="orphan_lane")) == "invalid"
        assert "no device model 'orphan_lane' is registered" in hiplib.lib().fabber_vb_last_error().decode()
        # with a wave body of that name the pair is a route
        sizes = re.search(r"KernelArgs 0 against (\d+) bytes, WaveLayout 0 against (\d+)\)", _wave_size_refusal())
        w = vbabi.FvbDeviceModel(b"orphan_lane", vbabi.FVB_ABI_VERSION, int(sizes.group(1)), int(sizes.group(2)), _never_launched_wave)
        hiplib.register_device_model(w)
        try:
            assert hiplib.kernel_name(invrec_config(name="orphan_lane")) == "lane<orphan_lane,3>"
        finally:
            hiplib.unregister_device_model("orphan_lane")
    finally:
        hiplib.unregister_device_lane_model("orphan_lane", 3)


def _wave_size_refusal():
    d = vbabi.FvbDeviceModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 0, _never_launched_wave)
    assert hiplib.lib().fabber_vb_register_device_model(C.byref(d)) == -72
    return hiplib.lib().fabber_vb_last_error().decode()
