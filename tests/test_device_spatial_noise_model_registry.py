"""Spatial VB kernels under AR(1) noise and noise patterns for the device bodies of model libraries, the part that needs
no GPU: the SDK header (include/fabber_device_spatial_noise_model.h) and the test library
(tests/plugins/fwdmodel_spatial_noise_models.hip) compile for gfx950, loading the library registers its (name, parameter
count) entries, the engine names the kernel table of a noise model exactly where it takes that route, and the registry
refuses what it must (fabber_vb_register_device_spatial_noise_model)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import device_model_lib
from fabber_core_amd import hiplib, vbabi

pytestmark = [pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]

AR1, PHIS = vbabi.SPATIAL_NOISE_AR1, vbabi.SPATIAL_NOISE_PHIS
AR = dict(noise=vbabi.NOISE_AR1, num_echoes=1)
SOURCE, PARTS, LIBRARY = "fwdmodel_spatial_noise_models.hip", (1, 2, 3, 4, 5), "libfabber_models_spatial_noise.so"
# rows of the state image for two parameters (vb_spatial.h, vb_spatial_noise.h): SpLayout<2>::ROWS plus the policy's own -
# 7 + 2 PT + 4 P + 4 under AR(1), 3 N + N PT + N P with N moment sets of a pattern (PT = P (P + 1) / 2)
EXTRA_AR1, EXTRA_PHIS2, EXTRA_PHIS4 = 7 + 2 * 3 + 4 * 2 + 4, 3 * 2 + 2 * 3 + 2 * 2, 3 * 4 + 4 * 3 + 4 * 2


@pytest.fixture(scope="module")
def library():
    path = device_model_lib.build(SOURCE, PARTS, LIBRARY)
    hiplib.load_model_library(path)
    return path


@vbabi.FvbDeviceSpatialNoiseModel.LAUNCH_FN
def _never_launched(kind, which, need_f, spatial_args, grid, lds_bytes, stream, err, err_len):
    return -1


def spatial_args_size():
    """sizeof(fvb::SpatialArgs) as the engine was compiled with it: its refusal of a descriptor with another size states it"""
    d = vbabi.FvbDeviceSpatialNoiseModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 3, AR1, 0, 0, 0, _never_launched)
    assert hiplib.lib().fabber_vb_register_device_spatial_noise_model(C.byref(d)) == -67
    return int(re.search(r"SpatialArgs 0 against (\d+) bytes", hiplib.lib().fabber_vb_last_error().decode()).group(1))


def descriptor(name, n_params=3, abi=vbabi.FVB_ABI_VERSION, spatial_args=None, families=AR1 | PHIS, launch=_never_launched, rows=(0, 0, 0)):
    d = vbabi.FvbDeviceSpatialNoiseModel()
    d.name = name.encode()
    d.abi_version = abi
    d.spatial_args_size = spatial_args_size() if spatial_args is None else spatial_args
    d.n_params = n_params
    d.families = families
    d.state_rows_ar1, d.state_rows_phis2, d.state_rows_phis4 = rows
    d.launch = launch
    return d


TWO = [dict(name="amp", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
       dict(name="r", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG)]


def config(name="multiexp_spn", params=TWO, V=256, T=21, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, dt=0.04, params=params,
                              param_overrides={params[0]["name"]: dict(type="M")}, **kw)


def test_descriptor_mirrors_the_header():
    """name, abi_version, spatial_args_size, n_params, families, the three row counts, launch - in the header's order, with
    the header's widths (a pointer, seven 32-bit members, a pointer: 48 bytes)"""
    fields = [f[0] for f in vbabi.FvbDeviceSpatialNoiseModel._fields_]
    assert fields == ["name", "abi_version", "spatial_args_size", "n_params", "families", "state_rows_ar1", "state_rows_phis2",
                      "state_rows_phis4", "launch"]
    assert C.sizeof(vbabi.FvbDeviceSpatialNoiseModel) == 8 + 7 * 4 + 4 + 8
    assert vbabi.FvbDeviceSpatialNoiseModel.launch.offset == 40
    header = open(os.path.join(device_model_lib.ROOT, "include", "fabber_vb.h")).read()
    struct = re.search(r"typedef struct fvb_device_spatial_noise_model\s*\{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"(\w+);", struct) == fields
    assert "#define FVB_SPATIAL_NOISE_AR1 %d\n" % AR1 in header and "#define FVB_SPATIAL_NOISE_PHIS %d\n" % PHIS in header
    assert (vbabi.SPNZ_WHITE, vbabi.SPNZ_PATTERN2, vbabi.SPNZ_PATTERN4, vbabi.SPNZ_AR1) == (0, 1, 2, 3)


def test_library_compiles_and_registers_its_entries(library):
    assert os.path.exists(library)
    assert {"multiexp_spn", "suppconv_sp"} <= set(hiplib.device_models())
    assert {("multiexp_spn", 2), ("suppconv_sp", 2)} <= set(hiplib.device_spatial_noise_models())
    assert {("multiexp_spn", 2), ("suppconv_sp", 2)} <= set(hiplib.device_spatial_models())
    assert "suppconv_sp" in hiplib.device_results_models() and "suppconv_sp" in hiplib.device_init_models()
    for name in ("multiexp_spn", "suppconv_sp"):
        e = hiplib.find_device_spatial_noise_model(name, 2)
        assert e.families == AR1 | PHIS and e.n_params == 2 and e.abi_version == vbabi.FVB_ABI_VERSION
        assert e.spatial_args_size == spatial_args_size()
        white = e.state_rows_ar1 - EXTRA_AR1  # SpLayout<2>::ROWS
        assert white > 0 and (e.state_rows_phis2, e.state_rows_phis4) == (white + EXTRA_PHIS2, white + EXTRA_PHIS4)
    assert hiplib.find_device_spatial_noise_model("multiexp_spn", 4) is None


def test_kernel_name_is_the_table_of_the_noise_model(library):
    for name in ("multiexp_spn", "suppconv_sp"):
        assert hiplib.spatial_kernel_name(config(name)) == "spatial<%s,2>" % name
        assert hiplib.spatial_kernel_name(config(name, **AR)) == "spatial<%s,2,ar1>" % name
        assert hiplib.spatial_kernel_name(config(name, need_f=True, **AR)) == "spatial<%s,2,ar1>" % name
        assert hiplib.spatial_kernel_name(config(name, noise_pattern="12")) == "spatial<%s,2,pattern2>" % name
        assert hiplib.spatial_kernel_name(config(name, noise_pattern="123")) == "spatial<%s,2,pattern4>" % name
        assert hiplib.spatial_kernel_name(config(name, noise_pattern="1234", need_f=True)) == "spatial<%s,2,pattern4>" % name
    supp = np.ones((21, 256))
    assert hiplib.spatial_kernel_name(config("suppconv_sp", suppdata=supp)) == "spatial<suppconv_sp,2>"
    assert hiplib.spatial_kernel_name(config("suppconv_sp", suppdata=supp, **AR)) == "spatial<suppconv_sp,2,ar1>"


def test_everything_else_has_no_kernel_table(library):
    assert hiplib.spatial_kernel_name(config(noise=vbabi.NOISE_AR1, num_echoes=2, T=22)) == ""
    assert hiplib.spatial_kernel_name(config(noise_pattern="12345")) == ""
    four = vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=2)
    assert hiplib.spatial_kernel_name(config(params=four, num_exps=2, **AR)) == ""  # (P = 4: no entry)


def test_registry_refuses_wrong_abi_size_counts_masks_and_duplicates(library):
    with pytest.raises(hiplib.HipEngineError, match="-66.*built for ABI version %d" % (vbabi.FVB_ABI_VERSION - 1)):
        hiplib.register_device_spatial_noise_model(descriptor("other_abi", abi=vbabi.FVB_ABI_VERSION - 1))
    with pytest.raises(hiplib.HipEngineError, match="-67.*struct size mismatch.*SpatialArgs %d against %d" % (spatial_args_size() + 8, spatial_args_size())):
        hiplib.register_device_spatial_noise_model(descriptor("other_args", spatial_args=spatial_args_size() + 8))
    for n in (0, 7):
        with pytest.raises(hiplib.HipEngineError, match="-65.*%d parameters .*1 to 6" % n):
            hiplib.register_device_spatial_noise_model(descriptor("other_count", n_params=n))
    for mask in (0, 4, AR1 | 8):
        with pytest.raises(hiplib.HipEngineError, match="-65.*families mask"):
            hiplib.register_device_spatial_noise_model(descriptor("other_mask", families=mask))
    with pytest.raises(hiplib.HipEngineError, match="-65.*longer than"):
        hiplib.register_device_spatial_noise_model(descriptor("n" * 200))
    with pytest.raises(hiplib.HipEngineError, match="-68.*'multiexp_spn' with 2 parameters are already registered"):
        hiplib.register_device_spatial_noise_model(descriptor("multiexp_spn", n_params=2))
    assert hiplib.lib().fabber_vb_register_device_spatial_noise_model(None) == -65
    no_launcher = descriptor("no_launcher", launch=vbabi.FvbDeviceSpatialNoiseModel.LAUNCH_FN())
    assert hiplib.lib().fabber_vb_register_device_spatial_noise_model(C.byref(no_launcher)) == -65
    assert "launcher is NULL" in hiplib.lib().fabber_vb_last_error().decode()
    assert not {"other_abi", "other_args", "other_count", "other_mask", "no_launcher"} & {n for n, _ in hiplib.device_spatial_noise_models()}


def test_register_and_unregister_an_entry(library):
    """another count of a registered name is an entry of its own; its mask and its row counts decide its routes; once it
    is gone the configuration has no kernel table again"""
    three = TWO + [dict(name="c", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY)]
    cfg = lambda **kw: config(params=three, **kw)
    assert hiplib.spatial_kernel_name(cfg(noise_pattern="12")) == ""
    two = hiplib.find_device_spatial_noise_model("multiexp_spn", 2)
    wrong = descriptor("multiexp_spn", n_params=3, families=PHIS, rows=(0, two.state_rows_phis2, two.state_rows_phis4))
    hiplib.register_device_spatial_noise_model(wrong)
    try:
        assert ("multiexp_spn", 3) in hiplib.device_spatial_noise_models()
        assert hiplib.find_device_spatial_noise_model("multiexp_spn", 3).families == PHIS
        # (rows compiled for another layout: the entry is there and is not taken)
        assert hiplib.spatial_kernel_name(cfg(noise_pattern="12")) == ""
        assert hiplib.spatial_kernel_name(cfg(**AR)) == ""
    finally:
        hiplib.unregister_device_spatial_noise_model("multiexp_spn", 3)
    assert ("multiexp_spn", 3) not in hiplib.device_spatial_noise_models() and ("multiexp_spn", 2) in hiplib.device_spatial_noise_models()
    with pytest.raises(hiplib.HipEngineError, match="-69.*'multiexp_spn' with 3 parameters"):
        hiplib.unregister_device_spatial_noise_model("multiexp_spn", 3)
    # an entry with the engine's row counts is taken for the families in its mask, and for those alone: a name that has a
    # wave body and the white-noise line only (tests/plugins/fwdmodel_spatial_models.hip)
    hiplib.load_model_library(device_model_lib.build_spatial_library())
    one_exp = dict(params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1), num_exps=1)
    assert hiplib.spatial_kernel_name(config("multiexp_sp", **one_exp, **AR)) == ""
    ar_only = descriptor("multiexp_sp", n_params=2, families=AR1, rows=(two.state_rows_ar1, 0, 0))
    hiplib.register_device_spatial_noise_model(ar_only)
    try:
        assert hiplib.spatial_kernel_name(config("multiexp_sp", **one_exp, **AR)) == "spatial<multiexp_sp,2,ar1>"
        assert hiplib.spatial_kernel_name(config("multiexp_sp", noise_pattern="12", **one_exp)) == ""  # (family not in its mask)
        assert hiplib.spatial_kernel_name(config("multiexp_sp", **one_exp)) == "spatial<multiexp_sp,2>"  # (the white entry's)
    finally:
        hiplib.unregister_device_spatial_noise_model("multiexp_sp", 2)
    assert hiplib.spatial_kernel_name(config("multiexp_sp", **one_exp, **AR)) == ""


def test_the_two_spatial_registries_do_not_see_each_other(library):
    """a name with FABBER_DEVICE_SPATIAL_MODEL lines only (tests/plugins/fwdmodel_spatial_models.hip) has no kernel table
    under AR(1) noise and patterns; an entry of the new registry alone gives none under white noise"""
    hiplib.load_model_library(device_model_lib.build_spatial_library())
    assert ("multiexp_sp", 2) in hiplib.device_spatial_models()
    assert "multiexp_sp" not in {n for n, _ in hiplib.device_spatial_noise_models()}
    assert hiplib.spatial_kernel_name(config("multiexp_sp", params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1),
                                             num_exps=1)) == "spatial<multiexp_sp,2>"
    for kw in (AR, dict(noise_pattern="12"), dict(noise_pattern="1234")):
        assert hiplib.spatial_kernel_name(config("multiexp_sp", params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1),
                                                 num_exps=1, **kw)) == ""
    four = vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=2)
    d = descriptor("multiexp_sp", n_params=3)
    hiplib.register_device_spatial_noise_model(d)
    try:
        assert ("multiexp_sp", 3) in hiplib.device_spatial_noise_models() and ("multiexp_sp", 3) not in hiplib.device_spatial_models()
        assert hiplib.spatial_kernel_name(config("multiexp_sp", params=TWO + four[:1])) == ""
    finally:
        hiplib.unregister_device_spatial_noise_model("multiexp_sp", 3)
