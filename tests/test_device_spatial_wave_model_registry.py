"""Wave-per-voxel spatial VB kernels for the device bodies of model libraries, the part that needs no GPU: the SDK header
(include/fabber_device_spatial_wave_model.h) and the test library (tests/plugins/fwdmodel_spatial_wave_models.hip) compile
for gfx950, loading the library registers its entries, the engine names the library's kernel table exactly where a run
would take it (fabber_vb_spatial_kernel_name), and the registry refuses what it must
(fabber_vb_register_device_spatial_wave_model)."""
import ctypes as C
import os
import re

import pytest

import device_model_lib
import device_spatial_wave_lib
from fabber_core_amd import hiplib, vbabi

pytestmark = [pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def library():
    path = device_spatial_wave_lib.build_spatial_wave_library()
    print("spatial wave model library: compile seconds per part %s"
          % {k: round(v, 1) for k, v in sorted(device_model_lib.seconds[device_spatial_wave_lib.LIBRARY].items())})
    hiplib.load_model_library(path)
    return path


@vbabi.FvbDeviceSpatialWaveModel.LAUNCH_FN
def _never_launched(which, need_f, spatial_args, grid, lds_bytes, stream, err, err_len):
    return -1


def engine_sizes():
    """sizeof(fvb::SpatialArgs), sizeof(fvb::WaveLayout) and the LDS probe as the engine was compiled with them: its refusal
    of a descriptor with other values states them"""
    d = vbabi.FvbDeviceSpatialWaveModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 0, 0, _never_launched)
    assert hiplib.lib().fabber_vb_register_device_spatial_wave_model(C.byref(d)) == -37
    m = re.search(r"SpatialArgs 0 against (\d+) bytes, WaveLayout 0 against (\d+), LDS doubles at FVB_MAX_PARAMS parameters 0 against (\d+)\)",
                  hiplib.lib().fabber_vb_last_error().decode())
    return tuple(int(g) for g in m.groups())


def descriptor(name, abi=vbabi.FVB_ABI_VERSION, spatial_args=None, wave_layout=None, probe=None):
    sizes = engine_sizes()
    d = vbabi.FvbDeviceSpatialWaveModel()
    d.name = name.encode()
    d.abi_version = abi
    d.spatial_args_size = sizes[0] if spatial_args is None else spatial_args
    d.wave_layout_size = sizes[1] if wave_layout is None else wave_layout
    d.lds_probe = sizes[2] if probe is None else probe
    d.launch = _never_launched
    return d


def multiexp_config(num_exps, name="multiexp_spw", V=210, T=21, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, num_exps=num_exps, dt=0.04,
                              params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **kw)


def test_field_order_is_the_headers():
    """the ctypes struct against the C struct of include/fabber_vb.h, field by field"""
    text = open(os.path.join(ROOT, "include", "fabber_vb.h")).read()
    body = re.search(r"typedef struct fvb_device_spatial_wave_model\s*\{(.*?)\}\s*fvb_device_spatial_wave_model;", text, re.S).group(1)
    fields = re.findall(r"^\s*(const char \*|int32_t |uint32_t |fvb_device_spatial_launch_fn )(\w+);", body, re.M)
    ctype = {"const char *": C.c_char_p, "int32_t ": C.c_int32, "uint32_t ": C.c_uint32,
             "fvb_device_spatial_launch_fn ": vbabi.FvbDeviceSpatialModel.LAUNCH_FN}
    assert [(n, ctype[t]) for t, n in fields] == list(vbabi.FvbDeviceSpatialWaveModel._fields_)
    assert [n for _, n in fields] == ["name", "abi_version", "spatial_args_size", "wave_layout_size", "lds_probe", "launch"]


def test_lds_probe_is_the_layouts_double_count():
    """sp_wave_layout(32) (csrc/vb_spatial_wave.h) and behind it the (2 P + 1) P parameter vectors and P doubles of rden:
    below the 64 KB a workgroup may have"""
    P, TC = 32, 64
    base = TC * (P | 1) + TC + 64 + 3 * P + P * (P + 1) // 2 + P + 6 + 5 * P + 2 * P * P
    assert engine_sizes()[2] == base + (2 * P + 1) * P + P and 8 * engine_sizes()[2] < 64 * 1024


def test_library_compiles_and_registers_its_entries(library):
    assert os.path.exists(library)
    names = {"multiexp_spw", "linear_spw", "suppconv_spw", "multiexp_both"}
    assert names <= set(hiplib.device_models()) and names <= set(hiplib.device_spatial_wave_models())
    assert ("multiexp_both", 2) in hiplib.device_spatial_models() and "multiexp_spw" not in [n for n, _ in hiplib.device_spatial_models()]
    entry = hiplib.find_device_spatial_wave_model("linear_spw")
    assert (entry.spatial_args_size, entry.wave_layout_size, entry.lds_probe) == engine_sizes() and entry.abi_version == vbabi.FVB_ABI_VERSION
    assert hiplib.find_device_spatial_wave_model("no_such_model") is None


def test_kernel_name_is_the_library_table_where_a_run_takes_it(library):
    for num in (1, 4, 5, 16):  # P = 2 (no lane entry of this name), 8, 10, 32
        assert hiplib.spatial_kernel_name(multiexp_config(num)) == "spatial<multiexp_spw,wave>"
        assert hiplib.spatial_kernel_name(multiexp_config(num, need_f=True)) == "spatial<multiexp_spw,wave>"
    # a lane entry for (name, P) comes first
    assert hiplib.spatial_kernel_name(multiexp_config(1, name="multiexp_both")) == "spatial<multiexp_both,2>"
    assert hiplib.spatial_kernel_name(multiexp_config(4, name="multiexp_both")) == "spatial<multiexp_both,wave>"
    # what keeps the host route (-40 from a run)
    assert hiplib.spatial_kernel_name(multiexp_config(5, noise_pattern="12")) == ""
    assert hiplib.spatial_kernel_name(multiexp_config(5, noise=vbabi.NOISE_AR1, num_echoes=1)) == ""
    assert hiplib.spatial_kernel_name(multiexp_config(17)) == ""  # (34 parameters: the table of fvb_config.params_ext)


def test_the_lane_registry_still_refuses_seven_parameters(library):
    """the new registry is a registry of its own: fvb_device_spatial_model is not widened"""
    d = vbabi.FvbDeviceSpatialModel(b"seven", vbabi.FVB_ABI_VERSION, engine_sizes()[0], 7, 0, _never_launched)
    with pytest.raises(hiplib.HipEngineError, match="-75.*7 parameters .*1 to 6"):
        hiplib.register_device_spatial_model(d)


def test_registry_refuses_wrong_abi_sizes_probe_and_duplicates(library):
    args, layout, probe = engine_sizes()
    with pytest.raises(hiplib.HipEngineError, match="-36.*built for ABI version %d" % (vbabi.FVB_ABI_VERSION - 1)):
        hiplib.register_device_spatial_wave_model(descriptor("other_abi", abi=vbabi.FVB_ABI_VERSION - 1))
    with pytest.raises(hiplib.HipEngineError, match="-37.*struct size mismatch \\(SpatialArgs %d against %d bytes" % (args + 8, args)):
        hiplib.register_device_spatial_wave_model(descriptor("other_args", spatial_args=args + 8))
    with pytest.raises(hiplib.HipEngineError, match="-37.*WaveLayout %d against %d," % (layout + 4, layout)):
        hiplib.register_device_spatial_wave_model(descriptor("other_layout", wave_layout=layout + 4))
    with pytest.raises(hiplib.HipEngineError, match="-37.*LDS doubles at FVB_MAX_PARAMS parameters %d against %d\\).*other kernel headers" % (probe - 32, probe)):
        hiplib.register_device_spatial_wave_model(descriptor("other_probe", probe=probe - 32))
    with pytest.raises(hiplib.HipEngineError, match="-38.*'linear_spw' are already registered"):
        hiplib.register_device_spatial_wave_model(descriptor("linear_spw"))
    assert hiplib.lib().fabber_vb_register_device_spatial_wave_model(None) == -35
    assert not {"other_abi", "other_args", "other_layout", "other_probe"} & set(hiplib.device_spatial_wave_models())


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
    h = multiexp_config(5, name="orphan_spw")
    assert hiplib.spatial_kernel_name(h) == ""
    d = descriptor("orphan_spw")
    hiplib.register_device_spatial_wave_model(d)
    try:
        assert "orphan_spw" in hiplib.device_spatial_wave_models()
        assert hiplib.spatial_kernel_name(h) == ""  # (an entry without a wave body of its name is never used)
        w, keep = _wave_body("orphan_spw")
        hiplib.register_device_model(w)
        try:
            assert hiplib.spatial_kernel_name(h) == "spatial<orphan_spw,wave>"
            hiplib.unregister_device_spatial_wave_model("orphan_spw")
            assert "orphan_spw" not in hiplib.device_spatial_wave_models() and "linear_spw" in hiplib.device_spatial_wave_models()
            assert hiplib.spatial_kernel_name(h) == ""
            with pytest.raises(hiplib.HipEngineError, match="-39.*'orphan_spw'"):
                hiplib.unregister_device_spatial_wave_model("orphan_spw")
        finally:
            hiplib.unregister_device_model("orphan_spw")
    finally:
        if "orphan_spw" in hiplib.device_spatial_wave_models():
            hiplib.unregister_device_spatial_wave_model("orphan_spw")
    assert hiplib.spatial_kernel_name(multiexp_config(5)) == "spatial<multiexp_spw,wave>"
