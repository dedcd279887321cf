"""Spatial VB around the device body of a model library under AR(1) noise and noise patterns, and with the voxel's
supplementary data (include/fabber_device_spatial_noise_model.h): the engine's set-up kernel and second sweep of every
noise policy compiled in the library's code object around the library's evaluator - against the CPU oracle with the
built-in kernels as control, the split first sweep against the per-level launches, the convolution body with a unit
impulse against the oracle's exponential model, per-voxel input curves through fabber_dorun against the host-model route
of the same library, device pointers, the initial-posterior kernel inside the run, too few supplementary rows, and what
stays refused (tests/plugins/fwdmodel_spatial_noise_models.hip: multiexp_spn, suppconv_sp).

The shapes are those of tests/test_device_spatial_model.py, the smallest at which these kernels can go wrong: a 7 x 6 x 5
volume masked to about 180 voxels has holes, missing neighbours, five z-planes for the slab sweep, two full wavefronts and
a partial one; 21 timepoints are no multiple of the 8-timepoint trip."""
import ctypes as C
import re

import numpy as np
import pytest

import device_model_lib
from fabber_core_amd import fabber, hiplib, vbabi
from test_device_model import initial_mvn
from test_device_spatial_model import DT, SHAPE, T, assert_routes_agree, exp_data, library_against_builtin_against_oracle, volume_of
from test_spatial import masked_volume

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]

AR = dict(noise=vbabi.NOISE_AR1, num_echoes=1)
# the noise models of a library's spatial entries: options, the tag of the kernel table
NOISES = {"ar1": (AR, "ar1"), "pattern 12": (dict(noise_pattern="12"), "pattern2"), "pattern 123": (dict(noise_pattern="123"), "pattern4"),
          "pattern 1234": (dict(noise_pattern="1234"), "pattern4")}
EXP_PARAMS = vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1)
PRIORS = {"M": (dict(param_overrides={"amp1": dict(type="M")}), {}),
          "M next to ARD with F": (dict(need_f=True, param_overrides={"amp1": dict(type="M"), "r1": dict(type="A")}), dict(check_f=True))}


@pytest.fixture(scope="module")
def library():
    assert hiplib.available() and hiplib.device_count() > 0
    path = device_model_lib.build("fwdmodel_spatial_noise_models.hip", (1, 2, 3, 4, 5), "libfabber_models_spatial_noise.so")
    hiplib.load_model_library(path)
    assert {("multiexp_spn", 2), ("suppconv_sp", 2)} <= set(hiplib.device_spatial_noise_models())
    assert {("multiexp_spn", 2), ("suppconv_sp", 2)} <= set(hiplib.device_spatial_models())
    return path


@pytest.fixture(scope="module")
def volume():
    mask, coords = masked_volume(SHAPE, seed=61, keep=0.85)
    V = coords.shape[1]
    assert 128 < V < 192 and len(set(coords[2].tolist())) == 5
    return mask, coords


def kernel_of(name, tag):
    return "spatial<%s,2%s>" % (name, "," + tag if tag else "")


def exp_pair(y, device_model, suppdata=None, **opts):
    """the same problem twice: for the oracle (and the built-in spatial kernels) as the exponential model, for the
    library's kernels as its body (same parameters, priors and initial posterior image)"""
    V = y.shape[1]
    ref = vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=1, dt=DT, **opts)
    mvn = initial_mvn(ref, y)
    ref = vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=1, dt=DT, init_mvn=mvn, **opts)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=device_model, num_exps=1, dt=DT, init_mvn=mvn, params=EXP_PARAMS,
                             suppdata=suppdata, **opts)
    return ref, dev


# ---- 1. multiexp_spn against the oracle, the built-in kernels as control ------------------------------------------------
@pytest.mark.parametrize("prior", sorted(PRIORS))
@pytest.mark.parametrize("noise", sorted(NOISES))
def test_multiexp_spn_against_the_oracle(library, volume, noise, prior):
    """The body computes the expression of the built-in exponential model, pointwise as the oracle does: parity.strict at
    its base tolerances, status and iteration counts the oracle's, no raised bound the built-in kernels do not need"""
    _, coords = volume
    noise_opts, tag = NOISES[noise]
    opts, kw = PRIORS[prior]
    y = exp_data(coords, 1, seed=62)
    ref, dev = exp_pair(y, "multiexp_spn", max_iterations=8, **noise_opts, **opts)
    library_against_builtin_against_oracle(ref, dev, vbabi.SpatialHolder(coords), y, "%s, %s" % (noise, prior), kernel_of("multiexp_spn", tag),
                                           kernel_of("exp", tag), **kw)


# ---- 2. the split first sweep ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["ar1", "pattern 12"])
def test_split_first_sweep_is_the_per_level_sweep_bit_for_bit(library, volume, noise, monkeypatch):
    """with F the prep kernel and the per-level kernel are the policy's own: the library's second sweep in the form that
    completes the split first sweep against its plain form after per-level launches, with the switches of the test of
    this name in tests/test_device_spatial_model.py"""
    _, coords = volume
    noise_opts, tag = NOISES[noise]
    y = exp_data(coords, 1, seed=64)
    _, dev = exp_pair(y, "multiexp_spn", max_iterations=6, need_f=True, param_overrides={"amp1": dict(type="M")}, **noise_opts)
    assert hiplib.spatial_kernel_name(dev) == kernel_of("multiexp_spn", tag)
    sp = vbabi.SpatialHolder(coords)
    forms = {}
    for name, env in (("default", {}), ("slabs of 1", {"FVB_SPATIAL_SLAB_DZ": "1"}), ("slabs of 2", {"FVB_SPATIAL_SLAB_DZ": "2"}),
                      ("slabs of 3", {"FVB_SPATIAL_SLAB_DZ": "3"}),
                      ("slab numbering on the host", {"FVB_SPATIAL_HOST_NUMBERING": "1"}),
                      ("prep kernel in index order", {"FVB_SPATIAL_PREP_LINEAR": "1"}),
                      ("geometry on the host", {"FVB_SPATIAL_HOST_GEOMETRY": "1"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        forms[name] = hiplib.run_spatial_host(dev, sp, y)
        for k in env:
            monkeypatch.delenv(k)
    monkeypatch.setenv("FVB_SPATIAL_PER_LEVEL", "1")
    per_level = hiplib.run_spatial_host(dev, sp, y)
    assert np.all(per_level["status"] == 0)
    for name, split in forms.items():
        for k in ("mvn", "status", "iterations", "free_energy"):
            assert np.array_equal(split[k], per_level[k], equal_nan=True), (noise, name, k)


# ---- 3. unit impulse: suppconv_sp is the built-in exponential model --------------------------------------------------------
@pytest.mark.parametrize("noise", ["white", "ar1", "pattern 12"])
def test_unit_impulse_against_the_oracle(library, volume, noise):
    """For supp = (1, 0, ...) in every voxel the convolution body computes the built-in exponential model's expression,
    term by term: held to the bounds of case 1"""
    _, coords = volume
    noise_opts, tag = NOISES[noise] if noise != "white" else ({}, "")
    assert kernel_of("suppconv_sp", NOISES["ar1"][1]) == "spatial<suppconv_sp,2,ar1>" and kernel_of("suppconv_sp", "") == "spatial<suppconv_sp,2>"
    y = exp_data(coords, 1, seed=62)
    supp = np.zeros((T, y.shape[1]))
    supp[0] = 1.0
    opts, kw = PRIORS["M next to ARD with F"]
    ref, dev = exp_pair(y, "suppconv_sp", suppdata=supp, max_iterations=8, **noise_opts, **opts)
    library_against_builtin_against_oracle(ref, dev, vbabi.SpatialHolder(coords), y, "unit impulse, " + noise, kernel_of("suppconv_sp", tag),
                                           kernel_of("exp", tag), **kw)


# ---- 4. the data reaches the right voxel -----------------------------------------------------------------------------------
def input_curves(V, rng):
    """[T][V]: input_curves of tests/test_device_supp_model.py for this file's 21 timepoints - a positive bump per voxel
    whose onset (0 .. 5 samples) and height differ from voxel to voxel, zero before the onset"""
    onset = rng.integers(0, 6, V)
    height = rng.uniform(0.5, 2.0, V)
    t = np.arange(T)[:, None]
    supp = height * np.exp(-0.5 * ((t - onset - 2.0) / 1.5) ** 2)
    return np.where(t >= onset, supp, 0.0)


def supp_series(coords, seed, dt=0.25, scale=100.0, noise_sd=2.0):
    """(supp [T][V], series [T][V] float32): supp_series of tests/test_device_supp_model.py with an amplitude that is
    smooth in space (amplitudes of order 100 with noise of 2: F stays away from zero)"""
    from test_device_supp_model import suppconv
    rng = np.random.default_rng(seed)
    V = coords.shape[1]
    supp = input_curves(V, rng)
    amp = scale * (1.0 + 0.15 * np.sin(coords[0] / 2.0) * np.cos(coords[1] / 3.0))
    clean = suppconv(supp, amp, rng.uniform(0.5, 1.5, V), dt=dt)
    return supp, (clean + rng.normal(0, noise_sd, clean.shape)).astype(np.float32)


@pytest.mark.parametrize("noise", ["white", "ar"])
def test_every_voxel_gets_its_own_input_curve_through_fabber_run(library, volume, noise):
    """method=spatialvb with per-voxel input curves: the device route against the host-model route of the same library,
    where the model's host code is handed each voxel's column. A curve from another voxel's column - another onset,
    another height - is far outside these bounds (the last assertion shows by how much).

    Eight iterations, the most these tests run: where supp_0 = 0 (five voxels in six) the amplitude starts at the prior
    mean 1 against a truth of order 100, and under AR(1) noise a few of the 174 voxels are still on their way after five -
    in the worst the rate's posterior variance is the prior's 4.6, the data weigh nothing yet, and the rounding differences of the
    two routes' linearisations (device exp against libm) show as 5e-6 in log r (median over the voxels 3e-10; through the C
    ABI with the same initial image, so not a matter of the host layer). After eight every voxel has settled (largest
    variance of log r 0.001) and the routes agree as under white noise. Measured on an MI355X: means and model fit equal
    in float32 under white noise; AR(1): noise 7.6e-6 relative, fit 3.1e-5 absolute, image 1.2e-5, F 3.0e-7."""
    from test_device_supp_model import assert_fit_images_agree
    mask, coords = volume
    supp, y = supp_series(coords, seed=71)
    data, supp_vol = volume_of(coords, y), volume_of(coords, supp.astype(np.float32))
    opts = {"model": "suppconv_sp", "dt": 0.25, "noise": noise, "method": "spatialvb", "param-spatial-priors": "MN", "max-iterations": 8,
            "save-mean": True, "save-mvn": True, "save-free-energy": True, "save-noise-mean": True, "save-model-fit": True,
            "save-residuals": True}
    m = mask.astype(np.int32)
    dev = fabber.run(data, opts, mask=m, extra_data={"suppdata": supp_vol}, model_libs=[library])
    host = fabber.run(data, dict(opts, **{"host-model": True}), mask=m, extra_data={"suppdata": supp_vol}, model_libs=[library])
    kernel = kernel_of("suppconv_sp", "ar1" if noise == "ar" else "")
    assert "with the body 'suppconv_sp' of its library, kernels %s" % kernel in dev["log"]
    assert "the body receives %d rows of supplementary data" % T in dev["log"]
    assert "(kernel init<suppconv_sp>)" in dev["log"] and "(kernel postproc<suppconv_sp>)" in dev["log"]
    assert "evaluated on the host" not in dev["log"]
    assert "evaluated on the host" in host["log"] and "of its library" not in host["log"]
    assert_routes_agree(dev, host, ("amp", "r"), mask)
    assert_fit_images_agree({k: dev[k][mask] for k in ("modelfit", "residuals")}, {k: host[k][mask] for k in ("modelfit", "residuals")}, data[mask])
    # the same volume with the curves handed to the wrong voxels (every column moved on by one)
    wrong = fabber.run(data, opts, mask=m, extra_data={"suppdata": volume_of(coords, np.roll(supp, 1, axis=1).astype(np.float32))},
                       model_libs=[library])
    assert np.abs(wrong["mean_amp"][mask] - host["mean_amp"][mask]).max() > 1e-2 * np.abs(host["mean_amp"][mask]).max()


# ---- 5. bit-identical pairs -------------------------------------------------------------------------------------------------
def supp_config(V, supp, **opts):
    SUPP_PARAMS = [dict(name="amp", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
                   dict(name="r", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG)]
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="suppconv_sp", dt=0.25, params=SUPP_PARAMS, suppdata=supp,
                              param_overrides={"amp": dict(type="M")}, **opts)


@pytest.mark.parametrize("noise", ["white", "ar1", "pattern 12"])
def test_device_pointers_and_the_init_kernel_inside_the_run_give_the_same_bits(library, volume, noise):
    """fabber_vb_run_spatial_device with the supplementary rows, the initial posterior and the noise classes on the device
    gives the bits of the host entry; a run without init_mvn - the library's initial-posterior kernel inside open(), which
    reads the rows too (amp = data_0 / supp_0) - gives the bits of the run that was given that kernel's image"""
    from fabber_core_amd.device import DeviceProblem
    _, coords = volume
    noise_opts, tag = NOISES[noise] if noise != "white" else ({}, "")
    supp, y = supp_series(coords, seed=72)
    V = y.shape[1]
    bare = supp_config(V, supp, max_iterations=5, need_f=True, **noise_opts)
    assert hiplib.spatial_kernel_name(bare) == kernel_of("suppconv_sp", tag) and hiplib.init_posterior_kernel_name(bare) == "init<suppconv_sp>"
    given = supp_config(V, supp, max_iterations=5, need_f=True, init_mvn=hiplib.init_posterior_host(bare, y), **noise_opts)
    sp = vbabi.SpatialHolder(coords)
    host = hiplib.run_spatial_host(given, sp, y)
    assert np.all(host["status"] == 0) and np.isfinite(host["mvn"]).all()
    prob = DeviceProblem(given, y, "cuda:0")
    prob.run_spatial(sp)
    dev = prob.results()
    inside = hiplib.run_spatial_host(bare, sp, y)
    for k in ("mvn", "status", "iterations", "free_energy"):
        assert np.array_equal(host[k], dev[k]), ("device pointers", k)
        assert np.array_equal(host[k], inside[k]), ("init kernel inside the run", k)


# ---- 6. fewer supplementary rows than timepoints ----------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["white", "ar1", "pattern 12"])
def test_too_few_rows_stop_every_voxel(library, volume, noise):
    """20 rows for 21 timepoints: the body's own bound check answers the timepoint without a row with a non-finite
    prediction - nothing is read past the block - the run returns and every voxel carries a non-zero status"""
    _, coords = volume
    noise_opts, tag = NOISES[noise] if noise != "white" else ({}, "")
    supp, y = supp_series(coords, seed=73)
    V = y.shape[1]
    whole = supp_config(V, supp, max_iterations=3, **noise_opts)
    mvn = hiplib.init_posterior_host(whole, y)
    short = supp_config(V, supp[:T - 1], max_iterations=3, init_mvn=mvn, **noise_opts)
    assert hiplib.spatial_kernel_name(short) == kernel_of("suppconv_sp", tag)
    r = hiplib.run_spatial_host(short, vbabi.SpatialHolder(coords), y)
    assert np.all(r["status"] != 0) and np.all(r["setup_failed"])
    ok = hiplib.run_spatial_host(supp_config(V, supp, max_iterations=3, init_mvn=mvn, **noise_opts), vbabi.SpatialHolder(coords), y)
    assert np.all(ok["status"] == 0)


# ---- 7. refusals and fall-backs ---------------------------------------------------------------------------------------------
def test_what_the_entries_do_not_cover_is_refused_as_before(library, volume):
    _, coords = volume
    V = coords.shape[1]
    y = exp_data(coords, 1, seed=62)
    for what, kw, n_times in (("two echoes", dict(noise=vbabi.NOISE_AR1, num_echoes=2), T + 1), ("five precisions", dict(noise_pattern="12345"), T)):
        ref = vbabi.build_config(vbabi.MODEL_EXP, V, n_times, num_exps=1, dt=DT, **kw)
        mvn = initial_mvn(ref, np.vstack([y, y[:1]])[:n_times])
        h = vbabi.build_config(vbabi.MODEL_PLUGIN, V, n_times, device_model="multiexp_spn", num_exps=1, dt=DT, init_mvn=mvn, params=EXP_PARAMS,
                               param_overrides={"amp1": dict(type="M")}, **kw)
        assert hiplib.spatial_kernel_name(h) == "", what
        with pytest.raises(hiplib.HipEngineError, match="-40.*no spatial kernel"):
            hiplib.run_spatial_host(h, vbabi.SpatialHolder(coords), np.vstack([y, y[:1]])[:n_times])
    # a kind outside the entry's mask: an entry for AR(1) alone (registered by hand, the launcher of the library's) under a pattern
    mine = hiplib.find_device_spatial_noise_model("multiexp_spn", 2)
    three = EXP_PARAMS + [dict(name="c", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY)]
    ar_only = vbabi.FvbDeviceSpatialNoiseModel(b"multiexp_spn", vbabi.FVB_ABI_VERSION, mine.spatial_args_size, 3, vbabi.SPATIAL_NOISE_AR1,
                                               mine.state_rows_ar1, 0, 0, mine.launch)
    hiplib.register_device_spatial_noise_model(ar_only)
    try:
        h = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_spn", num_exps=1, dt=DT, params=three, noise_pattern="12",
                               param_overrides={"amp1": dict(type="M")})
        assert hiplib.spatial_kernel_name(h) == ""
        with pytest.raises(hiplib.HipEngineError, match="-40.*no spatial kernel"):
            hiplib.run_spatial_host(h, vbabi.SpatialHolder(coords), y)
    finally:
        hiplib.unregister_device_spatial_noise_model("multiexp_spn", 3)


def test_the_launcher_refuses_a_kind_outside_its_mask(library):
    """called directly with the engine's number of a policy the macro line has no kernels for - white noise (the other
    header's), two echoes, 5 to 8 precisions - the launcher answers -40 with a message before anything is launched (a
    launch of these zeroed arguments would answer the launch error -100 - e or start a kernel)"""
    entry = hiplib.find_device_spatial_noise_model("multiexp_spn", 2)
    args, err = C.create_string_buffer(entry.spatial_args_size), C.create_string_buffer(512)
    for kind in (vbabi.SPNZ_WHITE, 4, 5, 6, 7, 99):
        rc = entry.launch(kind, 0, 0, C.cast(args, C.c_void_p), 1, 0, None, C.cast(err, C.c_void_p), len(err))
        assert rc == -40, kind
        assert re.search(r"'multiexp_spn' with 2 parameters: not compiled for noise kind %d \(its mask is 3\)" % kind, err.value.decode())


def test_a_library_with_the_white_line_alone_keeps_its_fall_backs(library):
    """the two pinned tests of the fall-back, run unmodified with this file's library loaded next to theirs:
    multiexp_sp (FABBER_DEVICE_SPATIAL_MODEL only) under noise=ar, suppconv (no spatial line at all) under spatial VB"""
    import test_device_spatial_model as white
    import test_device_supp_model as supp
    mask, coords = masked_volume(white.SHAPE, seed=61, keep=0.85)
    path = device_model_lib.build_spatial_library()
    hiplib.load_model_library(path)
    white.test_ar_noise_keeps_the_host_route(path, (mask, coords))
    supp_path = device_model_lib.build("fwdmodel_supp_models.hip", (1, 2, 3, 4, 5, 6), "libfabber_models_supp.so")
    hiplib.load_model_library(supp_path)
    supp.test_spatial_vb_falls_back_to_the_host_route(supp_path)
