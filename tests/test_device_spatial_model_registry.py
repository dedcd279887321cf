"""Spatial VB kernels for the device bodies of model libraries, the part that needs no GPU: the SDK header
(include/fabber_device_spatial_model.h) and the test library (tests/plugins/fwdmodel_spatial_models.hip) compile for
gfx950, loading the library registers its (name, parameter count) entries, the engine names the library's kernel table
exactly where a run would take it (fabber_vb_spatial_kernel_name), and the registry refuses what it must
(fabber_vb_register_device_spatial_model)."""
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
    path = device_model_lib.build_spatial_library()
    print("spatial model library: compile seconds per part %s" % {k: round(v, 1) for k, v in sorted(device_model_lib.seconds["libfabber_models_spatial.so"].items())})
    hiplib.load_model_library(path)
    return path


@vbabi.FvbDeviceSpatialModel.LAUNCH_FN
def _never_launched(which, need_f, spatial_args, grid, lds_bytes, stream, err, err_len):
    return -1


def spatial_args_size():
    """sizeof(fvb::SpatialArgs) as the engine was compiled with it: its refusal of a descriptor with another size states it"""
    d = vbabi.FvbDeviceSpatialModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 3, 0, _never_launched)
    assert hiplib.lib().fabber_vb_register_device_spatial_model(C.byref(d)) == -77
    return int(re.search(r"SpatialArgs 0 against (\d+) bytes", hiplib.lib().fabber_vb_last_error().decode()).group(1))


def descriptor(name, n_params=3, abi=vbabi.FVB_ABI_VERSION, spatial_args=None):
    d = vbabi.FvbDeviceSpatialModel()
    d.name = name.encode()
    d.abi_version = abi
    d.spatial_args_size = spatial_args_size() if spatial_args is None else spatial_args
    d.n_params = n_params
    d.state_rows = 0
    d.launch = _never_launched
    return d


INVREC_PARAMS = [dict(name="M0", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
                 dict(name="T1", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG),
                 dict(name="a", prior=(0.8, 4.0), post=(0.8, 1.0), prior_type="N", transform=vbabi.TRANSFORM_FRACTIONAL)]


def invrec_config(name="invrec_sp", V=210, T=12, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, constants=np.linspace(0.1, 3.0, T), params=INVREC_PARAMS, **kw)


def multiexp_config(num_exps, name="multiexp_sp", V=210, T=21, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, num_exps=num_exps, dt=0.04,
                              params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **kw)


def test_library_compiles_and_registers_its_entries(library):
    assert os.path.exists(library)
    assert {"multiexp_sp", "invrec_sp"} <= set(hiplib.device_models())
    assert {("multiexp_sp", 2), ("multiexp_sp", 4), ("invrec_sp", 3)} <= set(hiplib.device_spatial_models())


def test_kernel_name_is_the_library_table_where_a_run_takes_it(library):
    assert hiplib.spatial_kernel_name(multiexp_config(1)) == "spatial<multiexp_sp,2>"
    assert hiplib.spatial_kernel_name(multiexp_config(1, need_f=True)) == "spatial<multiexp_sp,2>"
    assert hiplib.spatial_kernel_name(multiexp_config(2)) == "spatial<multiexp_sp,4>"
    assert hiplib.spatial_kernel_name(invrec_config()) == "spatial<invrec_sp,3>"
    # what keeps the host route (-40 from a run)
    assert hiplib.spatial_kernel_name(multiexp_config(1, noise_pattern="12")) == ""
    assert hiplib.spatial_kernel_name(multiexp_config(1, noise=vbabi.NOISE_AR1, num_echoes=1)) == ""
    assert hiplib.spatial_kernel_name(multiexp_config(3)) == ""  # (P = 6: no entry)


def test_a_wave_body_without_spatial_entries_has_no_table(library):
    """the library of tests/plugins/fwdmodel_device_models.hip registers wave bodies only"""
    hiplib.load_model_library(device_model_lib.build_library())
    assert "multiexp_dev" in hiplib.device_models() and "multiexp_dev" not in [n for n, _ in hiplib.device_spatial_models()]
    assert hiplib.spatial_kernel_name(multiexp_config(1, name="multiexp_dev")) == ""


def test_built_in_models_name_their_own_tables(library):
    h = vbabi.build_config(vbabi.MODEL_EXP, 210, 21, num_exps=1, dt=0.04)
    assert hiplib.spatial_kernel_name(h) == "spatial<exp,2>"
    # (-44: noise models the spatial kernels do not run)
    ar = vbabi.build_config(vbabi.MODEL_EXP, 210, 21, num_exps=1, dt=0.04, noise=vbabi.NOISE_AR1, num_echoes=1)
    assert hiplib.spatial_kernel_name(ar) == "spatial<exp,2,ar1>"
    ar.cfg.ar_cross_terms = 1  # (one echo has no cross terms)
    assert hiplib.spatial_kernel_name(ar) == ""


def test_registry_refuses_wrong_abi_size_counts_and_duplicates(library):
    with pytest.raises(hiplib.HipEngineError, match="-76.*built for ABI version %d" % (vbabi.FVB_ABI_VERSION - 1)):
        hiplib.register_device_spatial_model(descriptor("other_abi", abi=vbabi.FVB_ABI_VERSION - 1))
    size = spatial_args_size()
    with pytest.raises(hiplib.HipEngineError, match="-77.*struct size mismatch \\(SpatialArgs %d against %d bytes\\)" % (size + 8, size)):
        hiplib.register_device_spatial_model(descriptor("other_args", spatial_args=size + 8))
    for n in (0, 7):
        with pytest.raises(hiplib.HipEngineError, match="-75.*%d parameters .*1 to 6" % n):
            hiplib.register_device_spatial_model(descriptor("other_count", n_params=n))
    with pytest.raises(hiplib.HipEngineError, match="-78.*'invrec_sp' with 3 parameters are already registered"):
        hiplib.register_device_spatial_model(descriptor("invrec_sp", n_params=3))
    assert hiplib.lib().fabber_vb_register_device_spatial_model(None) == -75
    assert not {"other_abi", "other_args", "other_count"} & {n for n, _ in hiplib.device_spatial_models()}


def state_rows(P):
    """fvb::SpLayout<P>::ROWS (vb_spatial.h): means, covariance, log-determinant, prior means and precisions, the two noise
    entries, J'J, J'r, r'r and the linearisation centre"""
    return 5 * P + P * (P + 1) + 4


def _wave_body(name):
    """a wave body of that name, never launched (the sizes as the engine's refusal of a probe states them)"""
    @vbabi.FvbDeviceModel.LAUNCH_FN
    def never(kernel_args, stream, err, err_len):
        return -1
    probe = vbabi.FvbDeviceModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 0, never)
    assert hiplib.lib().fabber_vb_register_device_model(C.byref(probe)) == -72
    sizes = re.search(r"KernelArgs 0 against (\d+) bytes, WaveLayout 0 against (\d+)\)", hiplib.lib().fabber_vb_last_error().decode())
    return vbabi.FvbDeviceModel(name.encode(), vbabi.FVB_ABI_VERSION, int(sizes.group(1)), int(sizes.group(2)), never), never


def test_an_entry_needs_a_wave_body_and_unregistering_returns_the_configuration_to_no_table(library):
    h = invrec_config(name="orphan_sp")
    assert hiplib.spatial_kernel_name(h) == ""
    d = descriptor("orphan_sp")
    d.state_rows = state_rows(3)
    hiplib.register_device_spatial_model(d)
    try:
        assert ("orphan_sp", 3) in hiplib.device_spatial_models()
        assert hiplib.spatial_kernel_name(h) == ""  # (an entry without a wave body of its name is never used)
        w, keep = _wave_body("orphan_sp")
        hiplib.register_device_model(w)
        try:
            assert hiplib.spatial_kernel_name(h) == "spatial<orphan_sp,3>"
            assert hiplib.spatial_kernel_name(invrec_config(name="orphan_sp", need_f=True)) == "spatial<orphan_sp,3>"
            hiplib.unregister_device_spatial_model("orphan_sp", 3)
            assert ("orphan_sp", 3) not in hiplib.device_spatial_models() and ("invrec_sp", 3) in hiplib.device_spatial_models()
            assert hiplib.spatial_kernel_name(h) == ""
            with pytest.raises(hiplib.HipEngineError, match="-79.*'orphan_sp' with 3 parameters"):
                hiplib.unregister_device_spatial_model("orphan_sp", 3)
            # an entry compiled for a state image with other rows than the engine's (another SpLayout) is no table
            d.state_rows = state_rows(3) + 1
            hiplib.register_device_spatial_model(d)
            assert hiplib.spatial_kernel_name(h) == ""
        finally:
            hiplib.unregister_device_model("orphan_sp")
    finally:
        if ("orphan_sp", 3) in hiplib.device_spatial_models():
            hiplib.unregister_device_spatial_model("orphan_sp", 3)
    assert hiplib.spatial_kernel_name(invrec_config()) == "spatial<invrec_sp,3>"
