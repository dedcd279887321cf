"""Wave-per-voxel spatial VB kernels under AR(1) noise for the device bodies of model libraries, the part that needs no GPU:
the SDK header (include/fabber_device_spatial_wave_ar_model.h) and the test library
(tests/plugins/fwdmodel_spatial_wave_ar_models.hip) compile for gfx950, loading the library registers its entries, the
engine names the library's kernel table exactly where a run would take it (fabber_vb_spatial_kernel_name), the registry
refuses what it must (fabber_vb_register_device_spatial_wave_ar_model), and the arithmetic of the state image and of the
LDS layouts."""
import ctypes as C
import os
import re

import pytest

import device_model_lib
import device_spatial_wave_ar_lib as arlib
from fabber_core_amd import hiplib, vbabi

pytestmark = [pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AR = arlib.AR


@pytest.fixture(scope="module")
def library():
    path = arlib.build_spatial_wave_ar_library()
    print("spatial wave AR model library: compile seconds per part %s"
          % {k: round(v, 1) for k, v in sorted(device_model_lib.seconds[arlib.LIBRARY].items())})
    hiplib.load_model_library(path)
    return path


@vbabi.FvbDeviceSpatialWaveArModel.LAUNCH_FN
def _never_launched(which, need_f, spatial_args, grid, lds_bytes, stream, err, err_len):
    return -1


PROBE_LABEL = "LDS doubles under AR\\(1\\) noise at FVB_MAX_PARAMS parameters"


def engine_sizes():
    """sizeof(fvb::SpatialArgs), sizeof(fvb::WaveLayout) and the LDS probe as the engine was compiled with them: its refusal
    of a descriptor with other values states them"""
    d = vbabi.FvbDeviceSpatialWaveArModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 0, 0, _never_launched)
    assert hiplib.lib().fabber_vb_register_device_spatial_wave_ar_model(C.byref(d)) == -88
    m = re.search(r"SpatialArgs 0 against (\d+) bytes, WaveLayout 0 against (\d+), %s 0 against (\d+)\)" % PROBE_LABEL,
                  hiplib.lib().fabber_vb_last_error().decode())
    return tuple(int(g) for g in m.groups())


def descriptor(name, abi=vbabi.FVB_ABI_VERSION, spatial_args=None, wave_layout=None, probe=None):
    sizes = engine_sizes()
    d = vbabi.FvbDeviceSpatialWaveArModel()
    d.name = name.encode()
    d.abi_version = abi
    d.spatial_args_size = sizes[0] if spatial_args is None else spatial_args
    d.wave_layout_size = sizes[1] if wave_layout is None else wave_layout
    d.lds_probe = sizes[2] if probe is None else probe
    d.launch = _never_launched
    return d


def multiexp_config(num_exps, name="multiexp_spwa", V=210, T=21, noise=AR, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, num_exps=num_exps, dt=0.04,
                              params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **noise, **kw)


# ---- layout arithmetic ----------------------------------------------------------------------------------------------------
def state_rows(P):
    """sp_wide_layout(P) followed by the rows of SpAr1<P>: 7 alpha rows, Ad and C, ud and uc, sd, sc, J1 and JT, r1, rT"""
    PT = P * (P + 1) // 2
    one_precision = P + PT + 1 + P + P + 1 + 1 + PT + P + 1 + P
    return one_precision + 7 + 2 * PT + 2 * P + 2 + 2 * P + 2


def model_layout_doubles(P, N):
    """sp_wave_model_layout(P, N) (csrc/vb_spatial_wave.h, vb_spatial_wave_model.h) as the parent has it"""
    TC = 64
    base = TC * (P | 1) + TC + 64 + 3 * P + N * (P * (P + 1) // 2 + P + 6) + 5 * P + 2 * P * P + ((TC + 16) // 2 if N > 1 else 0)
    return base + (2 * P + 1) * P + P


def test_state_image_rows():
    assert [state_rows(P) for P in (1, 7, 32)] == [28, 190, 2415]
    text = open(os.path.join(ROOT, "fabber_core_amd", "csrc", "vb_spatial_wave.h")).read()
    # the row order in the header is the order counted above
    order = re.search(r"R\.AL = S\.ROWS;(.*?)R\.ROWS = R\.RT \+ 1;", text, re.S).group(1)
    assert re.findall(r"R\.(\w+) =", order) == ["AD", "CC", "UD", "UC", "SD", "SC", "J1", "JT", "R1", "RT"]
    assert 8 * state_rows(32) == 19320  # bytes per voxel


def test_lds_probe_is_the_layouts_double_count():
    """sp_wave_ar_model_layout(32): sp_wave_model_layout(32) and behind it Ad and C [PT], ud, uc, J1, JT [4 P], the carried row
    [P + 1] and sd, sc, r1, rT: 67.5 KB of the 160 KB a workgroup may have"""
    P = 32
    PT = P * (P + 1) // 2
    want = model_layout_doubles(P, 1) + 2 * PT + 4 * P + (P + 1) + 4
    assert engine_sizes()[2] == want == 8443 and 8 * want == 67544 < 160 * 1024


def test_the_existing_layouts_are_the_parents():
    """the probes of the one-precision and pattern registries of the family - the double counts of sp_wave_model_layout(32)
    and sp_wave_model_layout(32, 8) - are the parent commit's: the AR areas lie behind them, in their own layout function"""
    import test_device_spatial_wave_noise_model_registry as pattern
    assert pattern.engine_sizes()[2] == model_layout_doubles(32, 8) == 11224
    d = vbabi.FvbDeviceSpatialWaveModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 0, 0, _never_launched)
    assert hiplib.lib().fabber_vb_register_device_spatial_wave_model(C.byref(d)) == -37
    m = re.search(r"LDS doubles at FVB_MAX_PARAMS parameters 0 against (\d+)\)", hiplib.lib().fabber_vb_last_error().decode())
    assert int(m.group(1)) == model_layout_doubles(32, 1) == 7222
    assert engine_sizes()[:2] == pattern.engine_sizes()[:2]  # (sizeof(SpatialArgs), sizeof(WaveLayout): one ABI)


def test_field_order_is_the_headers():
    """the ctypes struct against the C struct of include/fabber_vb.h, field by field; the codes it documents"""
    text = open(os.path.join(ROOT, "include", "fabber_vb.h")).read()
    body = re.search(r"typedef struct fvb_device_spatial_wave_ar_model\s*\{(.*?)\}\s*fvb_device_spatial_wave_ar_model;", text, re.S).group(1)
    fields = re.findall(r"^\s*(const char \*|int32_t |uint32_t |fvb_device_spatial_launch_fn )(\w+);", body, re.M)
    ctype = {"const char *": C.c_char_p, "int32_t ": C.c_int32, "uint32_t ": C.c_uint32,
             "fvb_device_spatial_launch_fn ": vbabi.FvbDeviceSpatialModel.LAUNCH_FN}
    assert [(n, ctype[t]) for t, n in fields] == list(vbabi.FvbDeviceSpatialWaveArModel._fields_)
    assert [n for _, n in fields] == ["name", "abi_version", "spatial_args_size", "wave_layout_size", "lds_probe", "launch"]
    assert "#define FVB_ABI_VERSION %d" % vbabi.FVB_ABI_VERSION in text and vbabi.FVB_ABI_VERSION == 11
    comment = text[:text.index("typedef struct fvb_device_spatial_wave_ar_model")].rsplit("/*", 1)[1]
    assert all("-%d" % code in comment for code in (86, 87, 88, 89, 96))


def test_library_compiles_and_registers_its_entries(library):
    assert os.path.exists(library)
    names = set(arlib.NAMES)
    assert names <= set(hiplib.device_models()) and names <= set(hiplib.device_spatial_wave_ar_models())
    # (the AR line requires neither the white line nor the pattern line)
    assert not names & set(hiplib.device_spatial_wave_models()) and not names & set(hiplib.device_spatial_wave_noise_models())
    assert ("multiexp_spwa_both", 4) in hiplib.device_spatial_noise_models()
    entry = hiplib.find_device_spatial_wave_ar_model("linear_spwa")
    assert (entry.spatial_args_size, entry.wave_layout_size, entry.lds_probe) == engine_sizes()
    assert entry.abi_version == vbabi.FVB_ABI_VERSION
    assert hiplib.find_device_spatial_wave_ar_model("no_such_model") is None


def test_kernel_name_is_the_library_table_where_a_run_takes_it(library):
    for num in (1, 2, 4, 5, 16):  # P = 2, 4, 8, 10, 32
        assert hiplib.spatial_kernel_name(multiexp_config(num)) == "spatial<multiexp_spwa,wave,ar1>"
        assert hiplib.spatial_kernel_name(multiexp_config(num, need_f=True)) == "spatial<multiexp_spwa,wave,ar1>"
    # white noise with one precision and a pattern on a name with only the AR line, and the table of fvb_config.params_ext
    assert hiplib.spatial_kernel_name(multiexp_config(5, noise={})) == ""
    assert hiplib.spatial_kernel_name(multiexp_config(5, noise=dict(noise_pattern="12"))) == ""
    assert hiplib.spatial_kernel_name(multiexp_config(17)) == ""  # (34 parameters)
    # two echoes and cross terms keep no table
    assert hiplib.spatial_kernel_name(multiexp_config(5, T=22, noise=dict(noise=vbabi.NOISE_AR1, num_echoes=2))) == ""
    for cross in ("same", "dual"):
        assert hiplib.spatial_kernel_name(multiexp_config(5, T=22, noise=dict(noise=vbabi.NOISE_AR1, num_echoes=2, ar_cross_terms=cross))) == ""
    # the lane entry wins at its count; the wave entry has the rest
    assert hiplib.spatial_kernel_name(multiexp_config(2, name="multiexp_spwa_both")) == "spatial<multiexp_spwa_both,4,ar1>"
    for num in (1, 3, 5, 16):
        assert hiplib.spatial_kernel_name(multiexp_config(num, name="multiexp_spwa_both")) == "spatial<multiexp_spwa_both,wave,ar1>"
    # the existing libraries' names have no kernels under AR(1) in this family, and the pattern registry's reserved bit stays refused
    import test_device_spatial_wave_noise_model_registry as pattern
    with pytest.raises(hiplib.HipEngineError, match="-24.*a family this engine does not know"):
        hiplib.register_device_spatial_wave_noise_model(pattern.descriptor("other_family", families=vbabi.SPATIAL_WAVE_NOISE_AR1))


def test_registry_refuses_wrong_abi_sizes_probe_and_duplicates(library):
    args, layout, probe = engine_sizes()
    with pytest.raises(hiplib.HipEngineError, match="-87.*built for ABI version %d" % (vbabi.FVB_ABI_VERSION - 1)):
        hiplib.register_device_spatial_wave_ar_model(descriptor("other_abi", abi=vbabi.FVB_ABI_VERSION - 1))
    with pytest.raises(hiplib.HipEngineError, match="-88.*struct size mismatch \\(SpatialArgs %d against %d bytes" % (args + 8, args)):
        hiplib.register_device_spatial_wave_ar_model(descriptor("other_args", spatial_args=args + 8))
    with pytest.raises(hiplib.HipEngineError, match="-88.*WaveLayout %d against %d," % (layout + 4, layout)):
        hiplib.register_device_spatial_wave_ar_model(descriptor("other_layout", wave_layout=layout + 4))
    with pytest.raises(hiplib.HipEngineError, match="-88.*%s %d against %d\\).*other kernel headers" % (PROBE_LABEL, probe - 32, probe)):
        hiplib.register_device_spatial_wave_ar_model(descriptor("other_probe", probe=probe - 32))
    # (the probe of the one-precision layout: a library compiled against headers without the AR areas)
    with pytest.raises(hiplib.HipEngineError, match="-88.*%s 7222 against %d\\)" % (PROBE_LABEL, probe)):
        hiplib.register_device_spatial_wave_ar_model(descriptor("other_probe", probe=7222))
    with pytest.raises(hiplib.HipEngineError, match="-89.*'linear_spwa' are already registered"):
        hiplib.register_device_spatial_wave_ar_model(descriptor("linear_spwa"))
    assert hiplib.lib().fabber_vb_register_device_spatial_wave_ar_model(None) == -86
    no_name = descriptor("x")
    no_name.name = None
    assert hiplib.lib().fabber_vb_register_device_spatial_wave_ar_model(C.byref(no_name)) == -86
    assert hiplib.lib().fabber_vb_unregister_device_spatial_wave_ar_model(None) == -86
    with pytest.raises(hiplib.HipEngineError, match="-96.*'no_such_model'"):
        hiplib.unregister_device_spatial_wave_ar_model("no_such_model")
    assert not {"other_abi", "other_args", "other_layout", "other_probe", "x"} & set(hiplib.device_spatial_wave_ar_models())


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
    h = multiexp_config(5, name="orphan_spwa")
    assert hiplib.spatial_kernel_name(h) == ""
    d = descriptor("orphan_spwa")
    hiplib.register_device_spatial_wave_ar_model(d)
    try:
        assert "orphan_spwa" in hiplib.device_spatial_wave_ar_models()
        assert hiplib.spatial_kernel_name(h) == ""  # (an entry without a wave body of its name is never used)
        w, keep = _wave_body("orphan_spwa")
        hiplib.register_device_model(w)
        try:
            assert hiplib.spatial_kernel_name(h) == "spatial<orphan_spwa,wave,ar1>"
            hiplib.unregister_device_spatial_wave_ar_model("orphan_spwa")
            assert "orphan_spwa" not in hiplib.device_spatial_wave_ar_models() and "linear_spwa" in hiplib.device_spatial_wave_ar_models()
            assert hiplib.spatial_kernel_name(h) == ""
            with pytest.raises(hiplib.HipEngineError, match="-96.*'orphan_spwa'"):
                hiplib.unregister_device_spatial_wave_ar_model("orphan_spwa")
            hiplib.register_device_spatial_wave_ar_model(d)  # re-registered: the route is back
            assert hiplib.spatial_kernel_name(h) == "spatial<orphan_spwa,wave,ar1>"
            hiplib.unregister_device_spatial_wave_ar_model("orphan_spwa")
        finally:
            hiplib.unregister_device_model("orphan_spwa")
    finally:
        if "orphan_spwa" in hiplib.device_spatial_wave_ar_models():
            hiplib.unregister_device_spatial_wave_ar_model("orphan_spwa")
    assert hiplib.spatial_kernel_name(multiexp_config(5)) == "spatial<multiexp_spwa,wave,ar1>"


def test_the_launcher_answers_too_few_lds_bytes_with_minus_40_and_starts_nothing(library):
    """the launcher's own check, called directly: 16 bytes of LDS are fewer than the layout of any P needs, and the bytes of the
    one-precision layout are fewer than the AR layout's, so it answers before it touches the device (grid, stream and the
    pointers in the arguments are never used) - and so it does for zeroed arguments, which are no launch of this family"""
    entry = hiplib.find_device_spatial_wave_ar_model("multiexp_spwa")
    h = multiexp_config(5)
    # SpatialArgs begins with KernelArgs, which begins with the configuration: a zeroed block with the configuration in front
    block, err = C.create_string_buffer(entry.spatial_args_size), C.create_string_buffer(512)
    assert entry.launch(0, 0, C.cast(block, C.c_void_p), 1, 16, None, C.cast(err, C.c_void_p), len(err)) == -40
    assert b"0 parameters with 16 bytes of LDS" in err.value
    C.memmove(block, C.byref(h.cfg), C.sizeof(h.cfg))
    one_precision = 8 * model_layout_doubles(10, 1)
    for which in (0, 1):
        for lds in (16, one_precision):
            assert entry.launch(which, 1, C.cast(block, C.c_void_p), 1, lds, None, C.cast(err, C.c_void_p), len(err)) == -40
            assert b"10 parameters with %d bytes of LDS is no launch of this family" % lds in err.value
    # a configuration the family does not cover: white noise
    white = multiexp_config(5, noise={})
    C.memmove(block, C.byref(white.cfg), C.sizeof(white.cfg))
    assert entry.launch(0, 1, C.cast(block, C.c_void_p), 1, 1 << 17, None, C.cast(err, C.c_void_p), len(err)) == -40
