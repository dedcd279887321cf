"""Lane-per-voxel kernels under AR(1) noise and noise patterns for the device bodies of model libraries, the part that
needs no GPU: the SDK header (include/fabber_device_lane_noise_model.h) and the test library
(tests/plugins/fwdmodel_lane_noise_models.hip) compile for gfx950, loading the library registers its (name, parameter
count) entries, the engine names the lane kernel of a family exactly where it takes that route, and the registry refuses
what it must (fabber_vb_register_device_lane_noise_model)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import device_lane_noise_lib
import device_model_lib
from fabber_core_amd import hiplib, vbabi

pytestmark = [pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]

AR1, PHIS = vbabi.LANE_NOISE_AR1, vbabi.LANE_NOISE_PHIS


@pytest.fixture(scope="module")
def library():
    path = device_lane_noise_lib.build_lane_noise_library()
    hiplib.load_model_library(path)
    return path


@vbabi.FvbDeviceLaneNoiseModel.LAUNCH_FN
def _never_launched(kernel_args, family, pattern_n, feed, lds_bytes, stream, err, err_len):
    return -1


def kernel_args_size():
    """sizeof(fvb::KernelArgs) as the engine was compiled with it: its refusal of a descriptor with another size states it"""
    d = vbabi.FvbDeviceLaneNoiseModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 3, AR1, 0, 0, 0, _never_launched)
    assert hiplib.lib().fabber_vb_register_device_lane_noise_model(C.byref(d)) == -72
    return int(re.search(r"KernelArgs 0 against (\d+) bytes", hiplib.lib().fabber_vb_last_error().decode()).group(1))


def descriptor(name, n_params=3, abi=vbabi.FVB_ABI_VERSION, kernel_args=None, families=AR1 | PHIS, launch=_never_launched):
    d = vbabi.FvbDeviceLaneNoiseModel()
    d.name = name.encode()
    d.abi_version = abi
    d.kernel_args_size = kernel_args_size() if kernel_args is None else kernel_args
    d.n_params = n_params
    d.families = families
    d.save_rows_ar1, d.save_rows_phis2, d.save_rows_phis4 = 37, 40, 60
    d.launch = launch
    return d


INVREC_PARAMS = [dict(name="M0", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
                 dict(name="T1", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG),
                 dict(name="a", prior=(0.8, 4.0), post=(0.8, 1.0), prior_type="N", transform=vbabi.TRANSFORM_FRACTIONAL)]
AR = dict(noise=vbabi.NOISE_AR1, num_echoes=1)


def invrec_config(name="invrec_lanenz", V=1 << 20, T=12, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, constants=np.linspace(0.1, 3.0, T), params=INVREC_PARAMS, **kw)


def multiexp_config(num_exps, V=1 << 20, T=50, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_lanenz", num_exps=num_exps, dt=0.04,
                              params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **kw)


def test_library_compiles_and_registers_its_entries(library):
    assert os.path.exists(library)
    assert {"multiexp_lanenz", "invrec_lanenz"} <= set(hiplib.device_models())
    assert device_lane_noise_lib.ENTRIES <= set(hiplib.device_lane_noise_models())
    assert device_lane_noise_lib.ENTRIES == {("multiexp_lanenz", 2), ("multiexp_lanenz", 4), ("invrec_lanenz", 3)}
    # the mask of a macro line and the rows of the save buffers of the families in it (3 P + P (P + 1) / 2 + 2 N + 2 for a
    # pattern kernel with N moment sets)
    ar_only, both = hiplib.find_device_lane_noise_model("multiexp_lanenz", 4), hiplib.find_device_lane_noise_model("invrec_lanenz", 3)
    assert ar_only.families == AR1 and ar_only.save_rows_ar1 > 0 and (ar_only.save_rows_phis2, ar_only.save_rows_phis4) == (0, 0)
    assert both.families == AR1 | PHIS and both.save_rows_ar1 > 0 and (both.save_rows_phis2, both.save_rows_phis4) == (21, 25)
    assert hiplib.find_device_lane_noise_model("multiexp_lanenz", 6) is None
    # (no FABBER_DEVICE_LANE_MODEL line: the white-noise registry does not know the names)
    assert not {"multiexp_lanenz", "invrec_lanenz"} & {n for n, _ in hiplib.device_lane_models()}


def test_kernel_name_is_the_lane_kernel_of_the_family(library):
    assert hiplib.kernel_name(invrec_config(**AR)) == "lane_ar1<invrec_lanenz,3>"
    assert hiplib.kernel_name(invrec_config(need_f=True, **AR)) == "lane_ar1<invrec_lanenz,3,F>"
    assert hiplib.kernel_name(invrec_config(noise_pattern="12")) == "lane_phis<invrec_lanenz,3,2>"
    assert hiplib.kernel_name(invrec_config(noise_pattern="12", need_f=True)) == "lane_phis<invrec_lanenz,3,2>"  # (F: a run-time switch)
    assert hiplib.kernel_name(invrec_config(noise_pattern="123")) == "lane_phis<invrec_lanenz,3,4>"
    assert hiplib.kernel_name(invrec_config(noise_pattern="1234")) == "lane_phis<invrec_lanenz,3,4>"
    assert hiplib.kernel_name(multiexp_config(1, **AR)) == "lane_ar1<multiexp_lanenz,2>"
    assert hiplib.kernel_name(multiexp_config(1, noise_pattern="12")) == "lane_phis<multiexp_lanenz,2,2>"
    assert hiplib.kernel_name(multiexp_config(2, need_f=True, **AR)) == "lane_ar1<multiexp_lanenz,4,F>"


def test_everything_else_keeps_the_wave_kernels(library):
    for variant in ("auto", "lane"):
        hiplib.set_variant(variant)
        try:
            assert hiplib.kernel_name(invrec_config(noise_pattern="12345")) == "wave<invrec_lanenz>"
            assert hiplib.kernel_name(invrec_config(noise=vbabi.NOISE_AR1, num_echoes=2)) == "wave<invrec_lanenz>"
            assert hiplib.kernel_name(invrec_config()) == "wave<invrec_lanenz>"  # (white, one precision: no white lane entry)
            assert hiplib.kernel_name(multiexp_config(2, noise_pattern="12")) == "wave<multiexp_lanenz>"  # (family not in its mask)
            assert hiplib.kernel_name(multiexp_config(3, **AR)) == "wave<multiexp_lanenz>"  # (P = 6: no entry)
            assert hiplib.kernel_name(multiexp_config(3, noise_pattern="12")) == "wave<multiexp_lanenz>"
        finally:
            hiplib.set_variant("auto")


def test_variant_wave_overrides_the_route(library):
    hiplib.set_variant("wave")
    try:
        assert hiplib.kernel_name(invrec_config(**AR)) == "wave<invrec_lanenz>"
        assert hiplib.kernel_name(invrec_config(noise_pattern="12")) == "wave<invrec_lanenz>"
    finally:
        hiplib.set_variant("auto")
    assert hiplib.kernel_name(invrec_config(**AR)) == "lane_ar1<invrec_lanenz,3>"


def test_patterns_follow_the_size_rule_of_the_builtin_kernels_and_ar1_has_none(library):
    """a small volume at or above 400 evaluations per pass (58 timepoints x 7 = 406) runs the wave kernels under a pattern,
    below that (12 x 7 = 84) or from 4096 voxels up the lane kernel; the built-in AR(1) kernels have no size rule, so the
    library's have none"""
    assert hiplib.kernel_name(invrec_config(V=64, T=58, noise_pattern="12")) == "wave<invrec_lanenz>"
    assert hiplib.kernel_name(invrec_config(V=4095, T=58, noise_pattern="12")) == "wave<invrec_lanenz>"
    assert hiplib.kernel_name(invrec_config(V=4096, T=58, noise_pattern="12")) == "lane_phis<invrec_lanenz,3,2>"
    assert hiplib.kernel_name(invrec_config(V=64, T=12, noise_pattern="12")) == "lane_phis<invrec_lanenz,3,2>"
    assert hiplib.kernel_name(invrec_config(V=64, T=58, **AR)) == "lane_ar1<invrec_lanenz,3>"
    hiplib.set_variant("lane")
    try:
        assert hiplib.kernel_name(invrec_config(V=64, T=58, noise_pattern="12")) == "lane_phis<invrec_lanenz,3,2>"
    finally:
        hiplib.set_variant("auto")


def test_registry_refuses_wrong_abi_size_counts_masks_and_duplicates(library):
    with pytest.raises(hiplib.HipEngineError, match="-71.*built for ABI version %d" % (vbabi.FVB_ABI_VERSION - 1)):
        hiplib.register_device_lane_noise_model(descriptor("other_abi", abi=vbabi.FVB_ABI_VERSION - 1))
    with pytest.raises(hiplib.HipEngineError, match="-72.*struct size mismatch.*KernelArgs %d against %d" % (kernel_args_size() + 8, kernel_args_size())):
        hiplib.register_device_lane_noise_model(descriptor("other_args", kernel_args=kernel_args_size() + 8))
    for n in (0, 7):
        with pytest.raises(hiplib.HipEngineError, match="-70.*%d parameters .*1 to 6" % n):
            hiplib.register_device_lane_noise_model(descriptor("other_count", n_params=n))
    for mask in (0, 4, AR1 | 8):
        with pytest.raises(hiplib.HipEngineError, match="-70.*families mask"):
            hiplib.register_device_lane_noise_model(descriptor("other_mask", families=mask))
    with pytest.raises(hiplib.HipEngineError, match="-73.*'invrec_lanenz' with 3 parameters are already registered"):
        hiplib.register_device_lane_noise_model(descriptor("invrec_lanenz", n_params=3))
    assert hiplib.lib().fabber_vb_register_device_lane_noise_model(None) == -70
    no_launcher = descriptor("no_launcher", launch=vbabi.FvbDeviceLaneNoiseModel.LAUNCH_FN())
    assert hiplib.lib().fabber_vb_register_device_lane_noise_model(C.byref(no_launcher)) == -70
    assert "launcher is NULL" in hiplib.lib().fabber_vb_last_error().decode()
    assert not {"other_abi", "other_args", "other_count", "other_mask", "no_launcher"} & {n for n, _ in hiplib.device_lane_noise_models()}


def test_register_and_unregister_an_entry(library):
    """another count of a registered name is an entry of its own, and its mask decides its routes; once it is gone the
    configuration names the wave kernels again"""
    five = [dict(name="p%d" % i, prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY) for i in range(5)]
    cfg = lambda **kw: vbabi.build_config(vbabi.MODEL_PLUGIN, 1 << 20, 12, device_model="invrec_lanenz", constants=np.linspace(0.1, 3.0, 12),
                                          params=five, **kw)
    assert hiplib.kernel_name(cfg(noise_pattern="12")) == "wave<invrec_lanenz>"
    d = descriptor("invrec_lanenz", n_params=5, families=PHIS)
    hiplib.register_device_lane_noise_model(d)
    try:
        assert ("invrec_lanenz", 5) in hiplib.device_lane_noise_models()
        assert hiplib.kernel_name(cfg(noise_pattern="12")) == "lane_phis<invrec_lanenz,5,2>"
        assert hiplib.kernel_name(cfg(**AR)) == "wave<invrec_lanenz>"
    finally:
        hiplib.unregister_device_lane_noise_model("invrec_lanenz", 5)
    assert ("invrec_lanenz", 5) not in hiplib.device_lane_noise_models() and ("invrec_lanenz", 3) in hiplib.device_lane_noise_models()
    assert hiplib.kernel_name(cfg(noise_pattern="12")) == "wave<invrec_lanenz>"
    with pytest.raises(hiplib.HipEngineError, match="-74.*'invrec_lanenz' with 5 parameters"):
        hiplib.unregister_device_lane_noise_model("invrec_lanenz", 5)


def test_the_white_noise_lane_entries_are_a_registry_of_their_own(library):
    """a name with FABBER_DEVICE_LANE_MODEL lines only (tests/plugins/fwdmodel_lane_models.hip) keeps the wave kernels under
    AR(1) noise and patterns"""
    hiplib.load_model_library(device_model_lib.build_lane_library())
    assert ("invrec_lane", 3) in hiplib.device_lane_models() and "invrec_lane" not in {n for n, _ in hiplib.device_lane_noise_models()}
    assert hiplib.kernel_name(invrec_config(name="invrec_lane", **AR)) == "wave<invrec_lane>"
    assert hiplib.kernel_name(invrec_config(name="invrec_lane", noise_pattern="12")) == "wave<invrec_lane>"
    assert hiplib.kernel_name(invrec_config(name="invrec_lane")) == "lane<invrec_lane,3>"
