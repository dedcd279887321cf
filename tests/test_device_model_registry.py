"""Device bodies supplied by model libraries, the part that needs no GPU: the SDK header (include/fabber_device_model.h)
and the test library (tests/plugins/fwdmodel_device_models.hip) compile for gfx950, loading the library registers its
bodies with the engine, and the registry refuses what it must (fabber_vb_register_device_model)."""
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
    path = device_model_lib.build_library()
    hiplib.load_model_library(path)
    return path


@vbabi.FvbDeviceModel.LAUNCH_FN
def _never_launched(kernel_args, stream, err, err_len):
    return -1


def engine_sizes():
    """sizeof(fvb::KernelArgs), sizeof(fvb::WaveLayout) as the engine was compiled with them: its refusal of a descriptor
    with other sizes states both"""
    d = vbabi.FvbDeviceModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 0, _never_launched)
    assert hiplib.lib().fabber_vb_register_device_model(C.byref(d)) == -72
    m = re.search(r"KernelArgs 0 against (\d+) bytes, WaveLayout 0 against (\d+)\)", hiplib.lib().fabber_vb_last_error().decode())
    return int(m.group(1)), int(m.group(2))


def descriptor(name, abi=vbabi.FVB_ABI_VERSION, kernel_args=None, wave_layout=None):
    ENGINE_SIZES = engine_sizes()
    d = vbabi.FvbDeviceModel()
    d.name = name.encode()
    d.abi_version = abi
    d.kernel_args_size = ENGINE_SIZES[0] if kernel_args is None else kernel_args
    d.wave_layout_size = ENGINE_SIZES[1] if wave_layout is None else wave_layout
    d.launch = _never_launched
    return d


def test_library_compiles_and_registers_its_bodies(library):
    assert os.path.exists(library)
    assert {"multiexp_dev", "invrec"} <= set(hiplib.device_models())


def test_registry_refuses_wrong_abi_sizes_and_duplicates(library):
    with pytest.raises(hiplib.HipEngineError, match="built for ABI version %d" % (vbabi.FVB_ABI_VERSION - 1)):
        hiplib.register_device_model(descriptor("other_abi", abi=vbabi.FVB_ABI_VERSION - 1))
    with pytest.raises(hiplib.HipEngineError, match="struct size mismatch"):
        hiplib.register_device_model(descriptor("other_args", kernel_args=engine_sizes()[0] + 8))
    with pytest.raises(hiplib.HipEngineError, match="struct size mismatch"):
        hiplib.register_device_model(descriptor("other_layout", wave_layout=engine_sizes()[1] - 4))
    with pytest.raises(hiplib.HipEngineError, match="'invrec' is already registered"):
        hiplib.register_device_model(descriptor("invrec"))
    assert not {"other_abi", "other_args", "other_layout"} & set(hiplib.device_models())


def test_register_and_unregister_a_name(library):
    d = descriptor("scratch_model")
    hiplib.register_device_model(d)
    try:
        assert "scratch_model" in hiplib.device_models()
    finally:
        hiplib.unregister_device_model("scratch_model")
    assert "scratch_model" not in hiplib.device_models()
    with pytest.raises(hiplib.HipEngineError, match="no device model 'scratch_model'"):
        hiplib.unregister_device_model("scratch_model")


def invrec_config(name="invrec", V=8, T=12, **kw):
    params = [dict(name="M0", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
              dict(name="T1", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG),
              dict(name="a", prior=(0.8, 4.0), post=(0.8, 1.0), prior_type="N", transform=vbabi.TRANSFORM_FRACTIONAL)]
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, constants=np.linspace(0.1, 3.0, T), params=params, **kw)


def test_unknown_name_fails_validation(library):
    h = invrec_config(name="no_such_model")
    assert hiplib.kernel_name(h) == "invalid"
    assert "no device model 'no_such_model' is registered" in hiplib.lib().fabber_vb_last_error().decode()
    h = invrec_config(name="")
    assert hiplib.kernel_name(h) == "invalid"


def test_kernel_name_names_the_body_whatever_the_size_and_variant(library):
    assert hiplib.kernel_name(invrec_config()) == "wave<invrec>"
    assert hiplib.kernel_name(invrec_config(V=1 << 20)) == "wave<invrec>"
    hiplib.set_variant("lane")
    try:
        assert hiplib.kernel_name(invrec_config()) == "wave<invrec>"
    finally:
        hiplib.set_variant("auto")


def test_config_carries_name_and_constants(library):
    h = invrec_config()
    assert h.cfg.model == vbabi.MODEL_PLUGIN and h.cfg.device_model == b"invrec"
    assert h.cfg.n_model_consts == 12 and h.cfg.model_consts == h.keep["constants"].ctypes.data
    assert h.cfg.n_params == 3 and h.cfg.transform[2] == vbabi.TRANSFORM_FRACTIONAL


def _refused_sizes(descriptor, register, code):
    """the struct sizes of the engine, in the order its refusal of a descriptor that states 0 for each names them"""
    assert register(C.byref(descriptor)) == code
    return [int(n) for n in re.findall(r"\w+ 0 against (\d+)", hiplib.lib().fabber_vb_last_error().decode())]


def test_the_four_registries_keep_their_entries_apart():
    """One name in all four registries (the NLLS one holds its wave entry next to the lane entry); taking it out of the
    lane registry leaves the other three as they were. Never-launched descriptors: no library, no GPU."""
    L, abi, name = hiplib.lib(), vbabi.FVB_ABI_VERSION, "apart_model"
    launch = {cls: cls.LAUNCH_FN(lambda *args: -1) for cls in (vbabi.FvbDeviceModel, vbabi.FvbDeviceLaneModel, vbabi.FvbDeviceNllsModel,
                                                                 vbabi.FvbDeviceSpatialModel)}
    wave_sizes = _refused_sizes(vbabi.FvbDeviceModel(b"size_probe", abi, 0, 0, launch[vbabi.FvbDeviceModel]), L.fabber_vb_register_device_model, -72)
    lane_sizes = _refused_sizes(vbabi.FvbDeviceLaneModel(b"size_probe", abi, 0, 3, 0, launch[vbabi.FvbDeviceLaneModel]),
                                L.fabber_vb_register_device_lane_model, -72)
    nlls_sizes = _refused_sizes(vbabi.FvbDeviceNllsModel(b"size_probe", abi, 0, 0, 3, launch[vbabi.FvbDeviceNllsModel]),
                                L.fabber_vb_register_device_nlls_model, -72)
    spatial_sizes = _refused_sizes(vbabi.FvbDeviceSpatialModel(b"size_probe", abi, 0, 3, 0, launch[vbabi.FvbDeviceSpatialModel]),
                                   L.fabber_vb_register_device_spatial_model, -77)
    assert (len(wave_sizes), len(lane_sizes), len(nlls_sizes), len(spatial_sizes)) == (2, 1, 2, 1)
    wave = vbabi.FvbDeviceModel(name.encode(), abi, wave_sizes[0], wave_sizes[1], launch[vbabi.FvbDeviceModel])
    lane = vbabi.FvbDeviceLaneModel(name.encode(), abi, lane_sizes[0], 3, 30, launch[vbabi.FvbDeviceLaneModel])
    nlls_wave = vbabi.FvbDeviceNllsModel(name.encode(), abi, nlls_sizes[0], nlls_sizes[1], 0, launch[vbabi.FvbDeviceNllsModel])
    nlls_lane = vbabi.FvbDeviceNllsModel(name.encode(), abi, nlls_sizes[0], nlls_sizes[1], 3, launch[vbabi.FvbDeviceNllsModel])
    spatial = vbabi.FvbDeviceSpatialModel(name.encode(), abi, spatial_sizes[0], 3, 0, launch[vbabi.FvbDeviceSpatialModel])
    undo = []
    try:
        hiplib.register_device_model(wave)
        undo.append(lambda: hiplib.unregister_device_model(name))
        hiplib.register_device_lane_model(lane)
        undo.append(lambda: hiplib.unregister_device_lane_model(name, 3))
        for d in (nlls_wave, nlls_lane):
            hiplib.register_device_nlls_model(d)
            undo.append(lambda n=d.n_params: hiplib.unregister_device_nlls_model(name, n))
        hiplib.register_device_spatial_model(spatial)
        undo.append(lambda: hiplib.unregister_device_spatial_model(name, 3))
        assert name in hiplib.device_models() and (name, 3) in hiplib.device_lane_models()
        assert {(name, 0), (name, 3)} <= set(hiplib.device_nlls_models()) and (name, 3) in hiplib.device_spatial_models()
        counts = (len(hiplib.device_models()), len(hiplib.device_nlls_models()), len(hiplib.device_spatial_models()))

        undo.pop(1)()  # the lane entry, and nothing else
        assert name not in [n for n, _ in hiplib.device_lane_models()]
        assert name in hiplib.device_models()
        assert {(name, 0), (name, 3)} <= set(hiplib.device_nlls_models())
        assert (name, 3) in hiplib.device_spatial_models()
        assert counts == (len(hiplib.device_models()), len(hiplib.device_nlls_models()), len(hiplib.device_spatial_models()))
    finally:
        for step in reversed(undo):
            step()
    assert name not in hiplib.device_models() and name not in [n for n, _ in hiplib.device_nlls_models() + hiplib.device_spatial_models()]
