"""Per-voxel supplementary data for the device body of a model library (fvb_config.model_supp, ModelArgs::supp,
fvb::supp_at): tests/plugins/fwdmodel_supp_models.hip's `suppconv` - an exponential residue function convolved with the
voxel's input curve - on the wave, lane, AR(1)-lane and NLLS kernels, the result-image and the initial-posterior kernel,
against the CPU oracle (unit impulse: the built-in exponential model), against itself with the voxels in another order
(also with the lane kernel's rescue forced, where a wavefront works on one voxel at a time), cut into blocks, through device pointers, and through fabber_dorun against the host-model route of the same library.

The shapes are the smallest at which this can go wrong: 197 voxels are three full wavefronts and five lanes of a fourth
(the lane kernels' lanes past the end repeat the last voxel), 16 or 21 timepoints, 1500 voxels in blocks of 256 for the
offset of a block's rows."""
import contextlib

import numpy as np
import pytest

import cases
import device_model_lib
import oracle
import parity
from fabber_core_amd import fabber, hiplib, vbabi

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]

T, DT = 16, 0.25
AR = dict(noise=vbabi.NOISE_AR1, num_echoes=1)
# SuppConvFwdModel::GetParameterDefaults
SUPP_PARAMS = [dict(name="amp", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
               dict(name="r", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG)]


@pytest.fixture(scope="module")
def library():
    assert hiplib.available() and hiplib.device_count() > 0
    path = device_model_lib.build("fwdmodel_supp_models.hip", (1, 2, 3, 4, 5, 6), "libfabber_models_supp.so")
    hiplib.load_model_library(path)
    assert "suppconv" in hiplib.device_models() and ("suppconv", 2) in hiplib.device_lane_models()
    assert {("suppconv", 0), ("suppconv", 2)} <= set(hiplib.device_nlls_models())
    assert "suppconv" in hiplib.device_results_models() and "suppconv" in hiplib.device_init_models()
    return path


@contextlib.contextmanager
def variant(name):
    hiplib.set_variant(name)
    try:
        yield
    finally:
        hiplib.set_variant("auto")


# ---- the problem ---------------------------------------------------------------------------------------------------
def input_curves(V, rng):
    """[T][V]: a positive bump per voxel whose onset (0 .. 5 samples) and height differ from voxel to voxel; zero before
    the onset, so that supp_0 == 0 for five voxels in six"""
    onset = rng.integers(0, 6, V)
    height = rng.uniform(0.5, 2.0, V)
    t = np.arange(T)[:, None]
    supp = height * np.exp(-0.5 * ((t - onset - 2.0) / 1.5) ** 2)
    return np.where(t >= onset, supp, 0.0)


def suppconv(supp, amp, r, dt=DT):
    """the model's expression for every voxel: [T][V]"""
    n = supp.shape[0]
    out = np.zeros(supp.shape)
    for t in range(n):
        for s in range(t + 1):
            out[t] += supp[s] * np.exp(-r * ((t - s) * dt))
    return amp * out


def supp_series(V, seed, scale=100.0, noise_sd=2.0, noise_free=()):
    """(supp [T][V] float64, series [T][V] float32, truth): amplitudes of order `scale` with noise of noise_sd - with the
    defaults F is of order -40, away from zero (assert_routes_agree of tests/test_device_model.py)"""
    rng = np.random.default_rng(seed)
    supp = input_curves(V, rng)
    truth = dict(amp=scale * rng.uniform(0.8, 1.2, V), r=rng.uniform(0.5, 1.5, V))
    clean = suppconv(supp, truth["amp"], truth["r"])
    y = clean + rng.normal(0, noise_sd, clean.shape)
    for v in noise_free:
        y[:, v] = clean[:, v]
    return supp, y.astype(np.float32), truth


def config(V, supp, **opts):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="suppconv", dt=DT, params=SUPP_PARAMS, suppdata=supp, **opts)


def supp_problem(V, seed, noise_free=(), **opts):
    """through the C ABI, with the initial posterior the library's own kernel writes (amp = data_0 / supp_0) given as
    init_mvn"""
    supp, y, _ = supp_series(V, seed, noise_free=noise_free)
    mvn = hiplib.init_posterior_host(config(V, supp, **opts), y)
    return config(V, supp, init_mvn=mvn, **opts), y


def same_bits(a, b, keys=("mvn", "free_energy", "status", "iterations")):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- 1. unit impulse: the built-in exponential model, against the oracle ----------------------------------------------
def impulse_pair(V, n_times, seed, f64=False, **opts):
    """the same problem twice: for the oracle as the built-in exponential model, for the library's kernels as suppconv
    with supp = (1, 0, 0, ...) in every voxel (same parameters, priors and initial posterior image)"""
    from test_device_model import initial_mvn
    ref, y = cases.exp_problem(V, n_times, 1, 0.04, seed=seed, **opts)
    if f64:
        y = y.astype(np.float64) + 1e-9  # (not representable in float32)
    mvn = initial_mvn(ref, y)
    ref, _ = cases.exp_problem(V, n_times, 1, 0.04, seed=seed, init_mvn=mvn, **opts)
    supp = np.zeros((n_times, V))
    supp[0] = 1.0
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, n_times, device_model="suppconv", dt=0.04, init_mvn=mvn, suppdata=supp,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1), **opts)
    return ref, dev, y


# (kernel variant, options, float64 series, the kernel's name)
IMPULSE_CASES = {
    "wave white,F": ("wave", dict(need_f=True), False, "wave<suppconv>"),
    "wave pattern 12,F": ("wave", dict(noise_pattern="12", need_f=True), False, "wave<suppconv>"),
    "wave ar1 one echo,F": ("wave", dict(need_f=True, **AR), False, "wave<suppconv>"),
    "lane white": ("lane", dict(), False, "lane<suppconv,2>"),  # float tiles
    "lane white,F": ("lane", dict(need_f=True), False, "lane<suppconv,2,F>"),
    "lane float64": ("lane", dict(need_f=True, convergence="trialmode"), True, "lane<suppconv,2,F>"),  # double tiles
    "lane masked timepoint": ("lane", dict(masked_timepoints=(5,)), False, "lane<suppconv,2>"),  # in-place feed
}


@pytest.mark.parametrize("case", sorted(IMPULSE_CASES))
def test_unit_impulse_against_the_oracle(library, case):
    """For supp = (1, 0, ...) the body computes the built-in exponential model's expression: held to the bounds
    tests/test_device_model.py and tests/test_device_lane_model.py hold multiexp_* to (parity.strict at its base
    tolerances, no raised floor; means within 1e-6; status and iteration counts equal)."""
    name, opts, f64, kernel = IMPULSE_CASES[case]
    ref, dev, y = impulse_pair(197, 21, seed=20260102, f64=f64, max_iterations=10, **opts)
    with variant(name):
        assert hiplib.kernel_name(dev) == kernel
        got = hiplib.run_host(dev, y)
    r = parity.strict(ref, oracle.run(ref, y), got, what="suppconv " + case, cpu2=oracle.run_fma(ref, y))
    print("suppconv %s: err means %.3e cov %.3e F %.3e" % (case, r["err_means"], r["err_cov"], r["err_f"]))
    assert not r["raised"]
    assert r["err_means"] < 1e-6


# ---- 2. per-voxel data reaches the right voxel ---------------------------------------------------------------------------
def reversed_problem(h, y, **opts):
    V = h.cfg.n_voxels
    back = config(V, np.ascontiguousarray(h.keep["suppdata"][:, ::-1]), init_mvn=np.ascontiguousarray(h.keep["init_mvn"][:, ::-1]), **opts)
    return back, np.ascontiguousarray(y[:, ::-1])


# four noise-free voxels, one per wavefront (where the moment form of k'k cancels the lane kernel takes its rescue; the
# test after this one forces it for every voxel)
NOISE_FREE = (3, 64, 130, 196)
ORDER_CASES = {"lane": ("lane", dict(need_f=True), "lane<suppconv,2,F>"),
               "wave": ("wave", dict(need_f=True), "wave<suppconv>"),
               "lane ar1": ("lane", dict(need_f=True, **AR), "lane_ar1<suppconv,2,F>")}


@pytest.mark.parametrize("case", sorted(ORDER_CASES))
def test_a_voxel_gets_its_own_input_curve_whatever_its_place(library, case):
    """197 voxels fitted, then fitted again in reverse order (series, supplementary data and initial posterior): every
    output of the second run is the reverse of the first, bit for bit - a voxel's result depends on nothing but that voxel
    (tests/test_device_lane_model.py::test_last_partial_wavefront), so a curve read from another voxel's column shows"""
    name, opts, kernel = ORDER_CASES[case]
    h, y = supp_problem(197, seed=61, noise_free=NOISE_FREE, max_iterations=6, **opts)
    back, y_back = reversed_problem(h, y, max_iterations=6, **opts)
    with variant(name):
        assert hiplib.kernel_name(h) == kernel
        a, b = hiplib.run_host(h, y), hiplib.run_host(back, y_back)
    assert np.all(a["status"] == 0)
    for k in ("mvn", "free_energy", "status", "iterations"):
        assert np.array_equal(a[k][..., ::-1], b[k], equal_nan=True), k
    # (and the curve matters: with every voxel given voxel 0's curve the fit is another one)
    same = np.repeat(h.keep["suppdata"][:, :1], 197, axis=1)
    other = config(197, same, init_mvn=h.keep["init_mvn"], max_iterations=6, **opts)
    with variant(name):
        c = hiplib.run_host(other, y)
    n = h.cfg.n_params + h.n_noise_outputs
    amp = n * (n + 1) // 2  # (the row of the amplitude's mean)
    assert np.array_equal(a["mvn"][:, 0], c["mvn"][:, 0]) and not np.allclose(a["mvn"][amp, 1:], c["mvn"][amp, 1:], rtol=1e-3)


@pytest.mark.parametrize("feed", ["tiles", "in place"])
def test_the_rescue_evaluates_the_body_with_the_rescued_voxels_curve(library, feed):
    """The lane kernel's rescue of k'k puts the whole wavefront on ONE voxel's series (64 timepoints at a time), so there
    every lane evaluates the body for another voxel than its own. With a residual tolerance of 1 every voxel takes the
    rescue in every iteration (k'k <= s + 2 |d'u| + |d'Ad| always): the fit is still the wave kernels' fit, and still the
    reverse of the fit in reverse order, bit for bit. Tile feeds take rescue_tiles; a masked timepoint, the in-place
    feed and rescue_residual."""
    from test_device_lane_model import assert_results_agree
    opts = dict(need_f=True, max_iterations=6, **({} if feed == "tiles" else dict(masked_timepoints=(5,))))
    h, y = supp_problem(197, seed=61, **opts)
    back, y_back = reversed_problem(h, y, **opts)
    with variant("wave"):
        wave = hiplib.run_host(h, y)
    hiplib.set_residual_tolerance(1.0)
    try:
        with variant("lane"):
            assert hiplib.kernel_name(h) == "lane<suppconv,2,F>"
            a, b = hiplib.run_host(h, y), hiplib.run_host(back, y_back)
    finally:
        hiplib.set_residual_tolerance(1e-10)  # (the engine's default, vb_api.hip)
    assert np.all(wave["status"] == 0)
    assert_results_agree(h, a, wave)
    for k in ("mvn", "free_energy", "status", "iterations"):
        assert np.array_equal(a[k][..., ::-1], b[k], equal_nan=True), k


def test_lane_against_wave(library):
    from test_device_lane_model import assert_results_agree
    h, y = supp_problem(197, seed=61, noise_free=NOISE_FREE, max_iterations=6, need_f=True)
    with variant("lane"):
        lane = hiplib.run_host(h, y)
    with variant("wave"):
        wave = hiplib.run_host(h, y)
    assert np.all(wave["status"] == 0)
    assert_results_agree(h, lane, wave)


# ---- 3. blocks -------------------------------------------------------------------------------------------------------------
def test_blocks_of_the_host_entry_point_get_their_own_rows(library, monkeypatch):
    """1500 voxels in blocks of 256 (the last one of 220) against the run in one block, and through the several-blocks
    entry point with the one device listed twice: a block reads the columns [v0, v1) of the supplementary rows. Without
    init_mvn: every block's initial-posterior kernel reads them too."""
    V = 1500
    supp, y, _ = supp_series(V, seed=62)
    h = config(V, supp, need_f=True, max_iterations=6)
    monkeypatch.setenv("FVB_HOST_BLOCK_VOXELS", "0")
    one = hiplib.run_host(h, y)
    assert np.all(one["status"] == 0)
    monkeypatch.setenv("FVB_HOST_BLOCK_VOXELS", "256")
    same_bits(one, hiplib.run_host(h, y))
    monkeypatch.setenv("FVB_HOST_BLOCK_VOXELS", "0")
    same_bits(one, hiplib.run_host(h, y, devices=[0, 0]))
    given = config(V, supp, need_f=True, max_iterations=6, init_mvn=hiplib.init_posterior_host(h, y))
    same_bits(one, hiplib.run_host(given, y))
    with variant("wave"):
        wave_one = hiplib.run_host(h, y)
        monkeypatch.setenv("FVB_HOST_BLOCK_VOXELS", "256")
        same_bits(wave_one, hiplib.run_host(h, y))


# ---- 4. device pointers ----------------------------------------------------------------------------------------------------
def test_device_pointers_take_the_supplementary_data_like_the_series(library):
    from fabber_core_amd.device import DeviceProblem
    h, y = supp_problem(256, seed=63, max_iterations=6, need_f=True)
    host = hiplib.run_host(h, y)
    prob = DeviceProblem(h, y, "cuda:0")
    assert prob.kernel == hiplib.kernel_name(h) == "lane<suppconv,2,F>"
    prob.run()
    dev = prob.results()
    same_bits(host, dev)
    assert np.all(host["status"] == 0)


# ---- 5. too few rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lane", "wave"])
def test_too_few_rows_stop_every_voxel_in_its_set_up(library, name):
    """15 rows for 16 timepoints, or no supplementary data at all: the body answers a timepoint without a row with a
    non-finite prediction - nothing is read past the block - and every voxel stops on the non-finite offset"""
    h, y = supp_problem(197, seed=64)
    for supp in (h.keep["suppdata"][:T - 1], None):
        short = config(197, supp, init_mvn=h.keep["init_mvn"])
        with variant(name):
            assert hiplib.kernel_name(short) == {"lane": "lane<suppconv,2>", "wave": "wave<suppconv>"}[name]
            r = hiplib.run_host(short, y)
        assert np.all(r["status"] == vbabi.STATUS_BAD_OFFSET) and np.all(r["setup_failed"])


def test_rows_announced_without_a_pointer_are_refused(library):
    h, y = supp_problem(64, seed=65)
    h.cfg.model_supp = None
    assert h.cfg.n_model_supp == T
    with pytest.raises(hiplib.HipEngineError, match="-17.*model_supp is NULL"):
        hiplib.run_host(h, y)
    h.cfg.model_supp = h.keep["suppdata"].ctypes.data
    h.cfg.n_model_supp = -1
    with pytest.raises(hiplib.HipEngineError, match="-17"):
        hiplib.run_host(h, y)


# ---- 6. through fabber_dorun against the host-model route -------------------------------------------------------------------
def volume(shape, seed, **kw):
    V = int(np.prod(shape))
    supp, y, truth = supp_series(V, seed, **kw)
    return y.T.reshape(shape + (T,)).copy(), supp.T.reshape(shape + (T,)).copy(), truth


def options(**extra):
    opts = {"model": "suppconv", "dt": DT, "noise": "white", "method": "vb", "max-iterations": 6, "save-mean": True, "save-mvn": True,
            "save-free-energy": True, "save-model-fit": True, "save-residuals": True}
    opts.update(extra)
    return opts


def both_routes(library, data, supp, opts):
    dev = fabber.run(data, opts, extra_data={"suppdata": supp}, model_libs=[library])
    host = fabber.run(data, dict(opts, **{"host-model": True}), extra_data={"suppdata": supp}, model_libs=[library])
    assert "with the body 'suppconv' of its library" in dev["log"]
    assert "the body receives %d rows of supplementary data" % T in dev["log"]
    assert "evaluated on the host" in host["log"] and "of its library" not in host["log"]
    return dev, host


def assert_fit_images_agree(dev, host, data):
    """the tolerances of tests/test_device_results_model.py"""
    assert np.allclose(host["modelfit"], dev["modelfit"], rtol=2e-5, atol=2e-5 * float(np.abs(data).max()))
    assert np.allclose(dev["modelfit"] + dev["residuals"], data, rtol=0, atol=1e-4)
    assert np.allclose(host["modelfit"] + host["residuals"], data, rtol=0, atol=1e-4)


@pytest.mark.parametrize("noise", ["white", "ar"])
def test_device_route_against_its_host_route(library, noise):
    from test_device_model import assert_routes_agree
    data, supp, _ = volume((6, 5, 4), seed=66)
    dev, host = both_routes(library, data, supp, options(noise=noise))
    kernel = {"white": "lane<suppconv,2,F>", "ar": "lane_ar1<suppconv,2,F>"}[noise]
    assert "kernel %s, 120 voxels x %d timepoints" % (kernel, T) in dev["log"]
    assert "(kernel init<suppconv>)" in dev["log"] and "(kernel postproc<suppconv>)" in dev["log"]
    assert_routes_agree(dev, host, ("mean_amp", "mean_r"))
    assert_fit_images_agree(dev, host, data)


def test_a_volume_that_takes_the_lane_kernels_by_the_size_rule(library):
    from test_device_model import assert_routes_agree
    data, supp, truth = volume((16, 16, 16), seed=67)
    dev, host = both_routes(library, data, supp, options())
    assert "kernel lane<suppconv,2,F>, 4096 voxels x %d timepoints" % T in dev["log"]
    assert_routes_agree(dev, host, ("mean_amp", "mean_r"))
    assert_fit_images_agree(dev, host, data)
    err = np.abs(dev["mean_amp"] - truth["amp"].reshape(16, 16, 16)) / truth["amp"].reshape(16, 16, 16)
    assert np.median(err) < 0.05  # (the fit is a fit)


def test_supplementary_data_missing_fails_cleanly_on_both_routes(library):
    data, _, _ = volume((4, 3, 2), seed=68)
    with pytest.raises(fabber.FabberError, match="Non-finite values found in offset"):
        fabber.run(data, options(), model_libs=[library])
    with pytest.raises(fabber.FabberError):
        fabber.run(data, options(**{"host-model": True}), model_libs=[library])


# ---- 7. method=nlls ---------------------------------------------------------------------------------------------------------
def test_nlls_device_route_against_its_host_route(library):
    """amplitudes of order 1, which the minimiser reaches from the parameters' initial posterior (amp = 1, r = 1) on
    both routes; the tolerances of tests/test_device_nlls_model.py"""
    from test_device_nlls_model import assert_routes_agree
    data, supp, truth = volume((6, 5, 4), seed=69, scale=1.0, noise_sd=0.02)
    opts = {"model": "suppconv", "dt": DT, "noise": "white", "method": "nlls", "save-mean": True, "save-mvn": True,
            "save-model-fit": True, "save-residuals": True}
    dev, host = both_routes(library, data, supp, opts)
    assert "kernel nlls" in dev["log"] and "<suppconv" in dev["log"]
    assert_routes_agree(dev, host, ("mean_amp", "mean_r"))
    assert np.allclose(dev["mean_amp"], truth["amp"].reshape(6, 5, 4), rtol=0.2)  # (the fit is a fit)
    assert np.allclose(dev["modelfit"] + dev["residuals"], data, rtol=0, atol=1e-4)
    assert np.allclose(host["modelfit"], dev["modelfit"], rtol=2e-5, atol=1e-5)


def test_nlls_lane_against_wave(library):
    """130 voxels: two full wavefronts and two lanes; the bound of test_invrec_lane_against_wave"""
    V, P = 130, 2
    supp, y, _ = supp_series(V, seed=70, scale=1.0, noise_sd=0.02)
    h = config(V, supp)
    res = {}
    for name, kernel in (("lane", "nlls<suppconv,2>"), ("wave", "nlls_wave<suppconv>")):
        with variant(name):
            assert hiplib.nlls_kernel_name(h) == kernel
            res[name] = hiplib.nlls_run_host(h, y, start=[1.0, 0.0])
    lane, wave = res["lane"], res["wave"]
    assert np.array_equal(lane["status"], wave["status"]) and np.all(wave["status"] == 0)
    sd = np.sqrt(np.stack([wave["mvn"][p * (p + 1) // 2 + p] for p in range(P)]))
    scale = np.maximum(np.abs(wave["mvn"][3:5]), sd)
    err = np.abs(lane["mvn"][3:5] - wave["mvn"][3:5]) / scale
    print("nlls<suppconv,2> against nlls_wave<suppconv>: means %.3e of max(|mean|, sd)" % err.max())
    assert err.max() <= 1e-4


# ---- 8. the initial posterior -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(), dict(**AR)], ids=["white", "ar1"])
def test_initial_posterior_is_the_host_loops_image(library, opts):
    """hiplib's init entry against Vb::BuildInitialMvn with SuppConvFwdModel::InitVoxelPosterior in NumPy, as
    tests/test_device_init_model.py compares them: amp = data_0 / supp_0 where supp_0 != 0, else the default"""
    from test_device_init_model import assert_image, numpy_image
    V = 197
    supp, y, _ = supp_series(V, seed=71)
    assert (supp[0] == 0).sum() > 20 and (supp[0] != 0).sum() > 5
    h = config(V, supp, **opts)
    assert hiplib.init_posterior_kernel_name(h) == "init<suppconv>"
    want, logs = numpy_image(h, y, "multiexp")
    n = h.cfg.n_params + h.n_noise_outputs
    with np.errstate(all="ignore"):
        want[n * (n + 1) // 2] = np.where(supp[0] != 0, y[0].astype(np.float64) / supp[0], 1.0)
    assert_image(hiplib.init_posterior_host(h, y), want, logs, "suppconv")


# ---- 9. spatial VB is the one route the supplementary data does not reach ---------------------------------------------------------
def test_spatial_vb_falls_back_to_the_host_route(library):
    data, supp, _ = volume((6, 5, 4), seed=72)
    opts = options(method="spatialvb", **{"param-spatial-priors": "MN", "max-iterations": 3})
    for k in ("save-free-energy", "save-model-fit", "save-residuals"):
        opts.pop(k)
    out = fabber.run(data, opts, extra_data={"suppdata": supp}, model_libs=[library])
    assert "the model is evaluated on the host" in out["log"] and "no supplementary data" in out["log"]
    forced = fabber.run(data, dict(opts, **{"host-model": True}), extra_data={"suppdata": supp}, model_libs=[library])
    assert np.array_equal(out["finalMVN"], forced["finalMVN"])
    # the C ABI refuses it with the code and text of a body without spatial kernels
    V = 4 * 4 * 4
    s, y, _ = supp_series(V, seed=73)
    h = config(V, s, init_mvn=hiplib.init_posterior_host(config(V, s), y), max_iterations=3, param_overrides={"amp": dict(type="M")})
    assert hiplib.spatial_kernel_name(h) == ""
    with pytest.raises(hiplib.HipEngineError, match="-40.*no spatial kernel"):
        hiplib.run_spatial_host(h, vbabi.SpatialHolder(vbabi.grid_coords((4, 4, 4))), y)
