"""Model fit and residuals from the device body of a model library (include/fabber_device_results_model.h): the engine's
result-image kernel compiled in the library's code object around the library's evaluator - at the engine's entry points
against the expression evaluated in NumPy at the means the SAME call returns, and through fabber_dorun against the host
loop of the same library (tests/plugins/fwdmodel_results_models.hip: multiexp_res, invrec_res).

The shapes are the smallest at which this kernel can go wrong: 300 voxels are one full workgroup of 256 lanes and a
partial one, and no multiple of 64; one voxel is a workgroup with one live lane; 34 parameters take the parameter table
and the kernel instance for up to FVB_MAX_PARAMS_EXT of them.

The tolerance of a fit against NumPy is the one the project holds "device exp against libm" to between its routes
(tests/test_device_model.py): rtol 2e-5, atol 2e-5 max|data|. Measured on an MI355X at the engine's entry points: max |fit - NumPy| 2.8e-14 on fits of
order 100 (invrec_res), 1.4e-14 for the 17 exponentials; through fabber.run, where the means are saved as float32, 9.8e-6
on a signal of 120 (invrec_res) and 1.1e-7 on one of 1.4 (multiexp_res)."""
import contextlib

import numpy as np
import pytest

import device_model_lib
import device_results_lib
from fabber_core_amd import fabber, hiplib, vbabi
from test_device_model import INVREC_PARAMS, TIS, assert_routes_agree, invrec_series

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]


@pytest.fixture(scope="module")
def library():
    assert hiplib.available() and hiplib.device_count() > 0
    path = device_results_lib.build_results_library()
    hiplib.load_model_library(path)
    assert {"multiexp_res", "invrec_res"} <= set(hiplib.device_results_models())
    return path


@pytest.fixture(scope="module")
def old_library():
    """wave bodies only (multiexp_dev, invrec): no results entry"""
    path = device_model_lib.build_library()
    hiplib.load_model_library(path)
    return path


def close_to_numpy(got, want, data, what):
    """rtol 2e-5, atol 2e-5 max|data|; the figure first"""
    scale = float(np.abs(data).max())
    print("%s: max |device - NumPy| %.3e (max|data| %.3e)" % (what, np.nanmax(np.abs(got - want)), scale))
    assert np.allclose(got, want, rtol=2e-5, atol=2e-5 * scale), what


# ---- the engine's entry points -----------------------------------------------------------------------------------
def invrec_images(V, seed, f64=False, constants=TIS, name="invrec_res"):
    """a result image with random finite means and positive variances (Fabber space: T1 = exp(.), a = logistic(.)), a
    random series of the order of the fit, and the configuration"""
    rng = np.random.default_rng(seed)
    T, P, n = len(TIS), 3, 4
    h = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, constants=constants, params=INVREC_PARAMS)
    nCov = n * (n + 1) // 2
    mvn = np.zeros((vbabi.mvn_rows(n), V))
    mvn[nCov + 0] = rng.uniform(50.0, 150.0, V)
    mvn[nCov + 1] = rng.uniform(-0.5, 0.5, V)
    mvn[nCov + 2] = rng.uniform(-1.0, 3.0, V)
    mvn[nCov + 3] = rng.uniform(0.1, 2.0, V)
    for q in range(n):
        mvn[q * (q + 1) // 2 + q] = rng.uniform(0.01, 2.0, V)
    mvn[-1] = 1.0
    y = rng.normal(0.0, 100.0, (T, V))
    return h, (y if f64 else y.astype(np.float32)), mvn


def invrec_numpy(mean, constants=TIS):
    """M0 (1 - 2 a exp(-TI / T1)) in float64 at model-space means [3][V]"""
    m0, t1, a = mean[0], mean[1], mean[2]
    return m0 * (1.0 - 2.0 * a * np.exp(-np.asarray(constants, dtype=np.float64)[:, None] / t1))


@pytest.mark.parametrize("V,f64", [(300, False), (300, True), (1, False)])
def test_invrec_fit_is_the_expression_at_the_means_of_the_same_call(library, V, f64):
    """Without a results entry (before the kernel could be compiled around a body) this configuration came back with two
    images of NaN and return code 0."""
    h, y, mvn = invrec_images(V, seed=101 + V, f64=f64)
    assert hiplib.postproc_kernel_name(h) == "postproc<invrec_res>"
    got = hiplib.postproc_host(h, y, mvn)
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["modelfit"]).all()
    close_to_numpy(got["modelfit"], invrec_numpy(got["mean"]), y, "invrec_res V=%d %s" % (V, "float64" if f64 else "float32"))
    assert np.array_equal(got["residuals"], y.astype(np.float64) - got["modelfit"])
    # the images that need no body are the engine's as ever
    assert np.array_equal(got["noise_mean"][0], mvn[4 * 5 // 2 + 3]) and np.array_equal(got["mean"][0], mvn[4 * 5 // 2])


def test_constants_shorter_than_the_series_give_nan_in_that_row_only(library):
    """15 inversion times for 16 timepoints: the body answers the timepoint without a constant with NaN - nothing is read
    past the constants block - and the image carries it, with its residual"""
    h, y, mvn = invrec_images(300, seed=111, constants=TIS[:-1])
    got = hiplib.postproc_host(h, y, mvn)
    assert np.isnan(got["modelfit"][15]).all() and np.isnan(got["residuals"][15]).all()
    want = invrec_numpy(got["mean"], TIS[:-1])
    close_to_numpy(got["modelfit"][:15], want, y, "invrec_res with 15 constants")
    assert np.array_equal(got["residuals"][:15], y[:15].astype(np.float64) - got["modelfit"][:15])


def multiexp_numpy(mean, T, dt):
    t = np.arange(T, dtype=np.float64)[:, None] * dt
    return sum(mean[2 * i] * np.exp(-mean[2 * i + 1] * t) for i in range(mean.shape[0] // 2))


def test_more_than_32_parameters_take_the_table_and_the_wide_instance(library):
    """17 exponentials: P = 34 - the per-parameter entries come from fvb_config.params_ext and the kernel is the instance
    for up to FVB_MAX_PARAMS_EXT parameters"""
    K, T, V, dt = 17, 8, 70, 0.1
    rng = np.random.default_rng(121)
    h = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_res", num_exps=K, dt=dt,
                           params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=K))
    P, n = 2 * K, 2 * K + 1
    assert P > vbabi.FVB_MAX_PARAMS and h.cfg.params_ext and hiplib.postproc_kernel_name(h) == "postproc<multiexp_res>"
    nCov = n * (n + 1) // 2
    mvn = np.zeros((vbabi.mvn_rows(n), V))
    for i in range(K):
        mvn[nCov + 2 * i] = rng.uniform(-2.0, 2.0, V)
        mvn[nCov + 2 * i + 1] = np.log(rng.uniform(0.5, 2.0, V))  # (rates are LOG-transformed)
    mvn[nCov + P] = 1.0
    for q in range(n):
        mvn[q * (q + 1) // 2 + q] = rng.uniform(0.01, 0.5, V)
    mvn[-1] = 1.0
    y = rng.normal(0.0, 5.0, (T, V)).astype(np.float32)
    got = hiplib.postproc_host(h, y, mvn)
    assert np.all((got["mean"][1::2] >= 0.5 * (1 - 1e-12)) & (got["mean"][1::2] <= 2.0 * (1 + 1e-12)))
    close_to_numpy(got["modelfit"], multiexp_numpy(got["mean"], T, dt), y, "multiexp_res with 17 exponentials")
    assert np.array_equal(got["residuals"], y.astype(np.float64) - got["modelfit"])


def test_device_pointers_give_the_bits_of_the_host_entry_point(library):
    """series, MVN, outputs and constants as torch device tensors (fabber_vb_postproc_device)"""
    import torch
    h, y, mvn = invrec_images(300, seed=401)
    host = hiplib.postproc_host(h, y, mvn)
    dev = hiplib.postproc_device(h, torch.from_numpy(y).to("cuda:0"), torch.from_numpy(mvn).to("cuda:0"))
    torch.cuda.synchronize()
    assert set(dev) == set(host)
    for k in host:
        assert np.array_equal(host[k], dev[k].cpu().numpy()), k


def test_a_body_without_a_results_entry_is_refused_not_answered_with_nan(library, old_library):
    h, y, mvn = invrec_images(300, seed=131, name="invrec")
    assert hiplib.postproc_kernel_name(h) == ""
    for want in (("modelfit",), ("residuals",), ("mean", "modelfit", "residuals")):
        with pytest.raises(hiplib.HipEngineError, match="-85.*'invrec'.*FABBER_DEVICE_RESULTS_MODEL"):
            hiplib.postproc_host(h, y, mvn, want=want)
    got = hiplib.postproc_host(h, y, mvn, want=("mean", "std"))  # (no body needed)
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["std"]).all()
    same, _, _ = invrec_images(300, seed=131)
    assert np.array_equal(got["mean"], hiplib.postproc_host(same, y, mvn, want=("mean",))["mean"])


@pytest.mark.parametrize("model", ["exp", "linear"])
def test_built_in_models_are_untouched(model):
    V, T = 300, 16
    rng = np.random.default_rng(141)
    if model == "exp":
        dt = 0.1
        h = vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=2, dt=dt)
        means = np.stack([rng.uniform(-2, 2, V), np.log(rng.uniform(0.5, 2.0, V)), rng.uniform(-2, 2, V), np.log(rng.uniform(0.5, 2.0, V))])
    else:
        design = rng.normal(0, 1, (T, 3))
        h = vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=design)
        means = rng.normal(0, 3, (3, V))
    assert hiplib.postproc_kernel_name(h) == "postproc"
    P, n = means.shape[0], means.shape[0] + 1
    nCov = n * (n + 1) // 2
    mvn = np.zeros((vbabi.mvn_rows(n), V))
    mvn[nCov:nCov + P] = means
    mvn[nCov + P] = 1.0
    for q in range(n):
        mvn[q * (q + 1) // 2 + q] = rng.uniform(0.01, 0.5, V)
    mvn[-1] = 1.0
    y = rng.normal(0.0, 5.0, (T, V)).astype(np.float32)
    got = hiplib.postproc_host(h, y, mvn)
    want = multiexp_numpy(got["mean"], T, dt) if model == "exp" else design @ got["mean"]
    close_to_numpy(got["modelfit"], want, y, "built-in " + model)
    assert np.array_equal(got["residuals"], y.astype(np.float64) - got["modelfit"])


# ---- through fabber_dorun ----------------------------------------------------------------------------------------
SHAPE = (6, 5, 4)
ROUTE_LINE = "model fit and residuals with the body '%s' of its library (kernel postproc<%s>)"
SAVE = {"save-mean": True, "save-model-fit": True, "save-residuals": True}


@contextlib.contextmanager
def variant(name):
    hiplib.set_variant(name)
    try:
        yield
    finally:
        hiplib.set_variant("auto")


def multiexp_volume(seed, T=40, dt=0.04, noise_sd=0.2):
    rng = np.random.default_rng(seed)
    t = np.arange(T) * dt
    amp = np.where(rng.random(SHAPE) < 0.5, 1.0, 0.5)
    rate = np.where(rng.random(SHAPE) < 0.5, 1.0, 0.8)
    return (amp[..., None] * np.exp(-rate[..., None] * t) + rng.normal(0, noise_sd, SHAPE + (T,))).astype(np.float32)


def fit_is_the_expression_at_the_saved_means(out, want, data):
    close_to_numpy(out["modelfit"], want, data, "modelfit against the saved means")
    assert np.allclose(out["modelfit"] + out["residuals"], data, rtol=0, atol=1e-4)


def test_invrec_res_under_vb(library):
    y, _ = invrec_series(120, seed=31, noise_sd=2.0)  # (the data of test_invrec_device_route_against_its_host_route)
    data = y.T.reshape(SHAPE + (len(TIS),)).copy()
    opts = dict(SAVE, **{"model": "invrec_res", "noise": "white", "method": "vb", "max-iterations": 6, "save-mvn": True,
                         "save-free-energy": True})
    for i, ti in enumerate(TIS):
        opts["ti%d" % (i + 1)] = float(ti)
    dev = fabber.run(data, opts, model_libs=[library])
    assert "kernel wave<invrec_res>" in dev["log"] and ROUTE_LINE % ("invrec_res", "invrec_res") in dev["log"]
    mean = np.stack([dev["mean_" + k].reshape(-1).astype(np.float64) for k in ("M0", "T1", "a")])
    fit_is_the_expression_at_the_saved_means(dev, invrec_numpy(mean).T.reshape(data.shape), data)
    # host-model: the host loop, no such line, and the two routes agree as the wave body's routes do
    host = fabber.run(data, dict(opts, **{"host-model": True}), model_libs=[library])
    assert "model fit and residuals with the body" not in host["log"] and "evaluated on the host" in host["log"]
    assert_routes_agree(dev, host, ("mean_M0", "mean_T1", "mean_a"))
    assert np.allclose(host["modelfit"], dev["modelfit"], rtol=2e-5, atol=2e-5 * float(np.abs(data).max()))
    assert np.allclose(host["modelfit"] + host["residuals"], data, rtol=0, atol=1e-4)


@pytest.mark.parametrize("method", ["vb", "spatialvb", "nlls"])
def test_multiexp_res_whatever_route_the_fit_took(library, method):
    """under spatial VB and NLLS this library has no kernels: the fit runs on the model's host code, the prediction at
    the fitted means still comes from the body"""
    data = multiexp_volume(seed=151)
    T, dt = data.shape[-1], 0.04
    opts = dict(SAVE, **{"model": "multiexp_res", "num-exps": 1, "dt": dt, "noise": "white", "method": method})
    if method != "nlls":
        opts["max-iterations"] = 5
    if method == "spatialvb":
        opts["param-spatial-priors"] = "MN"
    with variant("lane" if method == "vb" else "auto"):
        dev = fabber.run(data, opts, model_libs=[library])
        host = fabber.run(data, dict(opts, **{"host-model": True}), model_libs=[library])
    if method == "vb":
        assert "kernel lane<multiexp_res,2" in dev["log"]
    else:
        assert "evaluated on the host" in dev["log"]  # (the fit)
    assert ROUTE_LINE % ("multiexp_res", "multiexp_res") in dev["log"]
    mean = np.stack([dev["mean_" + k].reshape(-1).astype(np.float64) for k in ("amp1", "r1")])
    fit_is_the_expression_at_the_saved_means(dev, multiexp_numpy(mean, T, dt).T.reshape(data.shape), data)
    assert "model fit and residuals with the body" not in host["log"] and "evaluated on the host" in host["log"]
    for k in ("mean_amp1", "mean_r1"):
        assert np.allclose(host[k], dev[k], rtol=2e-5, atol=1e-5), k
    assert np.allclose(host["modelfit"], dev["modelfit"], rtol=2e-5, atol=2e-5 * float(np.abs(data).max()))
    assert np.allclose(host["modelfit"] + host["residuals"], data, rtol=0, atol=1e-4)


def test_a_library_without_a_results_entry_keeps_the_host_loop(library):
    lane = device_model_lib.build_lane_library()
    hiplib.load_model_library(lane)
    assert "multiexp_lane" in hiplib.device_models() and "multiexp_lane" not in hiplib.device_results_models()
    data = multiexp_volume(seed=151)
    opts = dict(SAVE, **{"model": "multiexp_lane", "num-exps": 1, "dt": 0.04, "noise": "white", "method": "vb", "max-iterations": 5})
    with variant("lane"):
        out = fabber.run(data, opts, model_libs=[lane])
        res = fabber.run(data, dict(opts, model="multiexp_res"), model_libs=[library])
    assert "kernel lane<multiexp_lane,2" in out["log"] and "model fit and residuals with the body" not in out["log"]
    assert np.allclose(out["modelfit"] + out["residuals"], data, rtol=0, atol=1e-4)
    # the same kernels fitted both: the same means, and the host loop's fit next to the body's
    for k in ("mean_amp1", "mean_r1"):
        assert np.allclose(out[k], res[k], rtol=2e-5, atol=1e-5), k
    assert np.allclose(out["modelfit"], res["modelfit"], rtol=2e-5, atol=2e-5 * float(np.abs(data).max()))
