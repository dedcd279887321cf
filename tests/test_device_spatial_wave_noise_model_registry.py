"""Wave-per-voxel spatial VB kernels under a noise pattern for the device bodies of model libraries, the part that needs no
GPU: the SDK header (include/fabber_device_spatial_wave_noise_model.h) and the test library
(tests/plugins/fwdmodel_spatial_wave_noise_models.hip) compile for gfx950, loading the library registers its entries, the
engine names the library's kernel table exactly where a run would take it (fabber_vb_spatial_kernel_name), and the registry
refuses what it must (fabber_vb_register_device_spatial_wave_noise_model)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import device_model_lib
import device_spatial_wave_noise_lib
from fabber_core_amd import hiplib, vbabi

pytestmark = [pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHIS = vbabi.SPATIAL_WAVE_NOISE_PHIS


@pytest.fixture(scope="module")
def library():
    path = device_spatial_wave_noise_lib.build_spatial_wave_noise_library()
    print("spatial wave noise model library: compile seconds per part %s"
          % {k: round(v, 1) for k, v in sorted(device_model_lib.seconds[device_spatial_wave_noise_lib.LIBRARY].items())})
    hiplib.load_model_library(path)
    return path


@vbabi.FvbDeviceSpatialWaveNoiseModel.LAUNCH_FN
def _never_launched(which, need_f, spatial_args, grid, lds_bytes, stream, err, err_len):
    return -1


PROBE_LABEL = "LDS doubles at FVB_MAX_PARAMS parameters and FVB_MAX_PHIS precisions"


def engine_sizes():
    """sizeof(fvb::SpatialArgs), sizeof(fvb::WaveLayout) and the LDS probe as the engine was compiled with them: its refusal
    of a descriptor with other values states them"""
    d = vbabi.FvbDeviceSpatialWaveNoiseModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 0, 0, PHIS, _never_launched)
    assert hiplib.lib().fabber_vb_register_device_spatial_wave_noise_model(C.byref(d)) == -26
    m = re.search(r"SpatialArgs 0 against (\d+) bytes, WaveLayout 0 against (\d+), %s 0 against (\d+)\)" % PROBE_LABEL,
                  hiplib.lib().fabber_vb_last_error().decode())
    return tuple(int(g) for g in m.groups())


def descriptor(name, abi=vbabi.FVB_ABI_VERSION, spatial_args=None, wave_layout=None, probe=None, families=PHIS):
    sizes = engine_sizes()
    d = vbabi.FvbDeviceSpatialWaveNoiseModel()
    d.name = name.encode()
    d.abi_version = abi
    d.spatial_args_size = sizes[0] if spatial_args is None else spatial_args
    d.wave_layout_size = sizes[1] if wave_layout is None else wave_layout
    d.lds_probe = sizes[2] if probe is None else probe
    d.families = families
    d.launch = _never_launched
    return d


def multiexp_config(num_exps, name="multiexp_spwn", V=210, T=21, noise_pattern="12", **kw):
    if noise_pattern is not None:
        kw["noise_pattern"] = noise_pattern
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, num_exps=num_exps, dt=0.04,
                              params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **kw)


def test_field_order_is_the_headers():
    """the ctypes struct against the C struct of include/fabber_vb.h, field by field"""
    text = open(os.path.join(ROOT, "include", "fabber_vb.h")).read()
    body = re.search(r"typedef struct fvb_device_spatial_wave_noise_model\s*\{(.*?)\}\s*fvb_device_spatial_wave_noise_model;", text, re.S).group(1)
    fields = re.findall(r"^\s*(const char \*|int32_t |uint32_t |fvb_device_spatial_launch_fn )(\w+);", body, re.M)
    ctype = {"const char *": C.c_char_p, "int32_t ": C.c_int32, "uint32_t ": C.c_uint32,
             "fvb_device_spatial_launch_fn ": vbabi.FvbDeviceSpatialModel.LAUNCH_FN}
    assert [(n, ctype[t]) for t, n in fields] == list(vbabi.FvbDeviceSpatialWaveNoiseModel._fields_)
    assert [n for _, n in fields] == ["name", "abi_version", "spatial_args_size", "wave_layout_size", "lds_probe", "families", "launch"]
    assert "#define FVB_SPATIAL_WAVE_NOISE_PHIS %d" % PHIS in text and "#define FVB_SPATIAL_WAVE_NOISE_AR1 %d" % vbabi.SPATIAL_WAVE_NOISE_AR1 in text


def test_lds_probe_is_the_layouts_double_count():
    """sp_wave_layout(32, 8) (csrc/vb_spatial_wave.h): the class areas 8-fold, the class lists of a chunk behind Sig, and
    behind that the (2 P + 1) P parameter vectors and P doubles of rden: 89.8 KB of the 160 KB a workgroup may have"""
    P, N, TC = 32, 8, 64
    base = TC * (P | 1) + TC + 64 + 3 * P + N * (P * (P + 1) // 2 + P + 6) + 5 * P + 2 * P * P + (TC + 16) // 2
    assert engine_sizes()[2] == base + (2 * P + 1) * P + P and 8 * engine_sizes()[2] == 89792 < 160 * 1024


def test_library_compiles_and_registers_its_entries(library):
    assert os.path.exists(library)
    names = set(device_spatial_wave_noise_lib.NAMES)
    assert names <= set(hiplib.device_models()) and names <= set(hiplib.device_spatial_wave_noise_models())
    assert not names & set(hiplib.device_spatial_wave_models())  # (the noise line does not require the white line)
    assert ("multiexp_spwn_both", 4) in hiplib.device_spatial_noise_models()
    entry = hiplib.find_device_spatial_wave_noise_model("linear_spwn")
    assert (entry.spatial_args_size, entry.wave_layout_size, entry.lds_probe) == engine_sizes()
    assert entry.abi_version == vbabi.FVB_ABI_VERSION and entry.families == PHIS
    assert hiplib.find_device_spatial_wave_noise_model("no_such_model") is None


def test_kernel_name_is_the_library_table_where_a_run_takes_it(library):
    for num in (1, 4, 5, 16):  # P = 2, 8, 10, 32
        for pattern in ("12", "123", "1234", "12345", "12345678"):
            want = "spatial<multiexp_spwn,wave,phis%d>" % len(pattern)
            assert hiplib.spatial_kernel_name(multiexp_config(num, noise_pattern=pattern)) == want
            assert hiplib.spatial_kernel_name(multiexp_config(num, noise_pattern=pattern, need_f=True)) == want
    # white noise with one precision on a name with only the noise line, AR(1), and the table of fvb_config.params_ext
    assert hiplib.spatial_kernel_name(multiexp_config(5, noise_pattern=None)) == ""
    assert hiplib.spatial_kernel_name(multiexp_config(5, noise_pattern=None, noise=vbabi.NOISE_AR1, num_echoes=1)) == ""
    assert hiplib.spatial_kernel_name(multiexp_config(17)) == ""  # (34 parameters)
    # the lane entry wins at its count under 2 to 4 precisions; the wave entry has the rest
    assert hiplib.spatial_kernel_name(multiexp_config(2, name="multiexp_spwn_both")) == "spatial<multiexp_spwn_both,4,pattern2>"
    assert hiplib.spatial_kernel_name(multiexp_config(2, name="multiexp_spwn_both", noise_pattern="123")) == "spatial<multiexp_spwn_both,4,pattern4>"
    assert hiplib.spatial_kernel_name(multiexp_config(2, name="multiexp_spwn_both", noise_pattern="12345")) == "spatial<multiexp_spwn_both,wave,phis5>"
    assert hiplib.spatial_kernel_name(multiexp_config(3, name="multiexp_spwn_both")) == "spatial<multiexp_spwn_both,wave,phis2>"


def test_nine_precisions_are_refused_before_the_route_is_asked(library):
    """"" from the selection function; a run is stopped by its argument checks (-5 n_phis out of range, which comes before
    the spatial entry points' own -44)"""
    h = multiexp_config(5, V=4, T=27, noise_pattern="123")
    assert hiplib.spatial_kernel_name(h) == "spatial<multiexp_spwn,wave,phis3>"
    h.cfg.n_phis = 9
    assert hiplib.spatial_kernel_name(h) == ""
    coords = np.array([[0, 1, 2, 3], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.int32)
    with pytest.raises(hiplib.HipEngineError, match="-5|-44"):
        hiplib.run_spatial_host(h, vbabi.SpatialHolder(coords), np.zeros((27, 4)))


def test_registry_refuses_wrong_abi_sizes_probe_masks_and_duplicates(library):
    args, layout, probe = engine_sizes()
    with pytest.raises(hiplib.HipEngineError, match="-25.*built for ABI version %d" % (vbabi.FVB_ABI_VERSION - 1)):
        hiplib.register_device_spatial_wave_noise_model(descriptor("other_abi", abi=vbabi.FVB_ABI_VERSION - 1))
    with pytest.raises(hiplib.HipEngineError, match="-26.*struct size mismatch \\(SpatialArgs %d against %d bytes" % (args + 8, args)):
        hiplib.register_device_spatial_wave_noise_model(descriptor("other_args", spatial_args=args + 8))
    with pytest.raises(hiplib.HipEngineError, match="-26.*WaveLayout %d against %d," % (layout + 4, layout)):
        hiplib.register_device_spatial_wave_noise_model(descriptor("other_layout", wave_layout=layout + 4))
    with pytest.raises(hiplib.HipEngineError, match="-26.*%s %d against %d\\).*other kernel headers" % (PROBE_LABEL, probe - 32, probe)):
        hiplib.register_device_spatial_wave_noise_model(descriptor("other_probe", probe=probe - 32))
    with pytest.raises(hiplib.HipEngineError, match="-24.*does not name FVB_SPATIAL_WAVE_NOISE_PHIS"):
        hiplib.register_device_spatial_wave_noise_model(descriptor("no_family", families=0))
    for mask in (vbabi.SPATIAL_WAVE_NOISE_AR1, PHIS | vbabi.SPATIAL_WAVE_NOISE_AR1, PHIS | 4):
        with pytest.raises(hiplib.HipEngineError, match="-24.*a family this engine does not know"):
            hiplib.register_device_spatial_wave_noise_model(descriptor("other_family", families=mask))
    with pytest.raises(hiplib.HipEngineError, match="-27.*'linear_spwn' are already registered"):
        hiplib.register_device_spatial_wave_noise_model(descriptor("linear_spwn"))
    assert hiplib.lib().fabber_vb_register_device_spatial_wave_noise_model(None) == -24
    assert not {"other_abi", "other_args", "other_layout", "other_probe", "no_family", "other_family"} & set(hiplib.device_spatial_wave_noise_models())


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
    h = multiexp_config(5, name="orphan_spwn")
    assert hiplib.spatial_kernel_name(h) == ""
    d = descriptor("orphan_spwn")
    hiplib.register_device_spatial_wave_noise_model(d)
    try:
        assert "orphan_spwn" in hiplib.device_spatial_wave_noise_models()
        assert hiplib.spatial_kernel_name(h) == ""  # (an entry without a wave body of its name is never used)
        w, keep = _wave_body("orphan_spwn")
        hiplib.register_device_model(w)
        try:
            assert hiplib.spatial_kernel_name(h) == "spatial<orphan_spwn,wave,phis2>"
            hiplib.unregister_device_spatial_wave_noise_model("orphan_spwn")
            assert "orphan_spwn" not in hiplib.device_spatial_wave_noise_models() and "linear_spwn" in hiplib.device_spatial_wave_noise_models()
            assert hiplib.spatial_kernel_name(h) == ""
            with pytest.raises(hiplib.HipEngineError, match="-28.*'orphan_spwn'"):
                hiplib.unregister_device_spatial_wave_noise_model("orphan_spwn")
            hiplib.register_device_spatial_wave_noise_model(d)  # re-registered: the route is back
            assert hiplib.spatial_kernel_name(h) == "spatial<orphan_spwn,wave,phis2>"
            hiplib.unregister_device_spatial_wave_noise_model("orphan_spwn")
        finally:
            hiplib.unregister_device_model("orphan_spwn")
    finally:
        if "orphan_spwn" in hiplib.device_spatial_wave_noise_models():
            hiplib.unregister_device_spatial_wave_noise_model("orphan_spwn")
    assert hiplib.spatial_kernel_name(multiexp_config(5)) == "spatial<multiexp_spwn,wave,phis2>"


def test_the_launcher_answers_too_few_lds_bytes_with_minus_40_and_starts_nothing(library):
    """the launcher's own check, called directly as tests/test_device_spatial_noise_model.py calls the lane launcher: 16 bytes
    of LDS are fewer than the layout of any (P, N) needs, so it answers before it touches the device (grid, stream and the
    pointers in the arguments are never used) - and so it does for zeroed arguments, which are no launch of this family"""
    entry = hiplib.find_device_spatial_wave_noise_model("multiexp_spwn")
    h = multiexp_config(5)
    # SpatialArgs begins with KernelArgs, which begins with the configuration: a zeroed block with the configuration in front
    block, err = C.create_string_buffer(entry.spatial_args_size), C.create_string_buffer(512)
    assert entry.launch(0, 0, C.cast(block, C.c_void_p), 1, 16, None, C.cast(err, C.c_void_p), len(err)) == -40
    assert b"0 parameters and 0 noise precisions with 16 bytes of LDS" in err.value
    C.memmove(block, C.byref(h.cfg), C.sizeof(h.cfg))
    for which in (0, 1):
        assert entry.launch(which, 1, C.cast(block, C.c_void_p), 1, 16, None, C.cast(err, C.c_void_p), len(err)) == -40
        assert b"10 parameters and 2 noise precisions with 16 bytes of LDS is no launch of this family" in err.value
