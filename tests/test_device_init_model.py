"""The initial posterior of a model library's device body on the GPU (include/fabber_device_init_model.h): the kernel the
library compiled around its body's init_posterior writes the image the fit kernels read as init_mvn
(tests/plugins/fwdmodel_init_models.hip: multiexp_init, invrec_init; multiexp_noinit has a wave body and no entry).

Three things are held:
  - the image is Vb::BuildInitialMvn's, restated in NumPy: EXACTLY in every row whose value involves IEEE-exact operations
    only (identity-transformed means and variances, the FRACTIONAL variance, zeros, the noise rows, the last row), and to
    4 ulp in the rows that take a logarithm (LOG means and variances, FRACTIONAL means: log(1 / m - 1), whose argument is
    the same bits on both sides). Either side's log is within 1 ulp of the true value, so they are within 2 ulp of each
    other; doubled as margin. No softplus parameter here: its variance transform cancels and no bound can be derived;
  - every route that fits consumes it: a run without init_mvn and a run given the image of init_posterior_device are the
    same input bits through the same kernels, so their outputs are bit-identical;
  - fabber_dorun takes the route, says so in its log, and agrees with the host classes of libraries without an entry to
    the tolerances tests/test_device_model.py holds the device route to against the host route.

The shapes are the kernel's edges: 1 voxel (one live lane), 63 and 65 (below and above a wavefront), 257 (one past a
256-lane workgroup); 1 and 17 timepoints. Two echoes of AR(1) noise need an even series: 18 timepoints there (the engine
refuses 17 with -6, as the reference does)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import device_init_lib
import device_model_lib
from fabber_core_amd import fabber, hiplib, vbabi
from test_device_model import INVREC_PARAMS, TIS, assert_routes_agree, invrec_series

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]


@pytest.fixture(scope="module")
def library():
    assert hiplib.available() and hiplib.device_count() > 0
    path = device_init_lib.build_init_library()
    hiplib.load_model_library(path)
    assert {"multiexp_init", "invrec_init"} <= set(hiplib.device_init_models())
    assert "multiexp_noinit" in hiplib.device_models() and "multiexp_noinit" not in hiplib.device_init_models()
    return path


@contextlib.contextmanager
def variant(name):
    hiplib.set_variant(name)
    try:
        yield
    finally:
        hiplib.set_variant("auto")


# ---- Vb::BuildInitialMvn in NumPy --------------------------------------------------------------------------------
def numpy_image(h, y, model):
    """(image [rows][V], the rows that took a logarithm): FwdModel::GetInitialPosterior with the InitVoxelPosterior of the
    test library's host class, FwdModel::ToFabber, the noise model's initial posterior, as inference_vb.cc scatters them"""
    cfg = h.cfg
    V, P, N = cfg.n_voxels, cfg.n_params, cfg.n_phis
    NA = 2 + cfg.ar_cross_terms if cfg.noise == vbabi.NOISE_AR1 else 0
    n = P + NA + N
    nCov = n * (n + 1) // 2
    tab = h.keep["param_table"][0] if cfg.params_ext else None

    def entry(field, k):
        return tab[field][k] if tab is not None else getattr(cfg, field)[k]
    y64 = np.asarray(y, dtype=np.float64)
    means, variances = np.empty((P, V)), np.empty((P, V))
    for i in range(P):
        means[i] = h.keep["image_%d" % i] if entry("prior_type", i) == vbabi.PRIOR_IMAGE else entry("post_mean", i)
        variances[i] = entry("post_var", i)
    if model == "multiexp":  # posterior.means(1) = data(1)
        means[0] = y64[0]
    else:  # m = fabs(data(t)) > m ? fabs(data(t)) : m; if (m > 0) posterior.means(1) = m
        m = np.zeros(V)
        with np.errstate(invalid="ignore"):
            for t in range(y64.shape[0]):
                a = np.abs(y64[t])
                m = np.where(a > m, a, m)
        means[0] = np.where(m > 0, m, means[0])
    img = np.zeros((vbabi.mvn_rows(n), V))
    logs = []
    with np.errstate(all="ignore"):
        for i in range(P):
            tr, d = entry("transform", i), i * (i + 1) // 2 + i
            if tr == vbabi.TRANSFORM_LOG:
                img[nCov + i], img[d] = np.log(means[i]), np.log(variances[i])
                logs += [nCov + i, d]
            elif tr == vbabi.TRANSFORM_FRACTIONAL:
                img[nCov + i], img[d] = np.log(1 / means[i] - 1), variances[i]
                logs += [nCov + i]
            else:
                assert tr == vbabi.TRANSFORM_IDENTITY
                img[nCov + i], img[d] = means[i], variances[i]
    for a in range(NA):
        q = P + a
        if cfg.ar_alpha_given & 2:
            for a2 in range(a + 1):
                img[q * (q + 1) // 2 + P + a2] = cfg.ar_alpha_post_cov[a][a2]
            img[nCov + q] = cfg.ar_alpha_post_mean[a]
        else:
            img[q * (q + 1) // 2 + q] = 1e4
    for k in range(N):
        b, c = cfg.noise_post_b[k], cfg.noise_post_c[k]
        q = P + NA + k
        img[q * (q + 1) // 2 + q] = b * b * c
        img[nCov + q] = b * c
    img[-1] = 1.0
    return img, sorted(logs)


def assert_image(got, want, logs, what):
    """exact outside the rows of `logs`, 4 ulp of the NumPy value inside; the figure first"""
    assert got.shape == want.shape, what
    exact = np.ones(want.shape[0], dtype=bool)
    exact[logs] = False
    with np.errstate(invalid="ignore"):
        ulps = np.abs(got[logs] - want[logs]) / np.spacing(np.abs(want[logs]))
    same = (got[logs] == want[logs]) | (np.isnan(got[logs]) & np.isnan(want[logs]))
    ulps = np.where(same, 0.0, ulps)
    print("%s: %d rows exact, %d rows with a logarithm: largest difference %.2f ulp" % (what, exact.sum(), len(logs), ulps.max() if ulps.size else 0))
    assert np.array_equal(got[exact], want[exact], equal_nan=True), what
    assert np.all(ulps <= 4.0), what  # (a NaN on one side only is a NaN here: refused)


def series(V, T, f64, seed):
    """a series of order 100 with, from 63 voxels up, one voxel of all zeros (keeps the default mean) and one with a NaN
    sample (not the first one where there is another: the comparison of the largest magnitude skips it)"""
    rng = np.random.default_rng(seed)
    y = rng.normal(0.0, 100.0, (T, V))
    if V >= 63:
        y[:, 3] = 0.0
        y[min(1, T - 1), 5] = np.nan
    return y if f64 else y.astype(np.float32)


def invrec_config(V, T, name="invrec_init", **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, constants=np.linspace(0.1, 4.0, T), params=INVREC_PARAMS, **kw)


def multiexp_params(num_exps):
    """MultiExpFwdModel::GetParameterDefaults (tests/plugins/test_device_models.h): the amplitudes untransformed, the rates
    LOG-transformed"""
    params = []
    for i in range(num_exps):
        params.append(dict(name="amp%d" % (i + 1), prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY))
        params.append(dict(name="r%d" % (i + 1), prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG))
    return params


def multiexp_config(V, T, num_exps=1, name="multiexp_init", dt=0.04, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, num_exps=num_exps, dt=dt, params=multiexp_params(num_exps), **kw)


def device_image(h, y):
    import torch
    img = hiplib.init_posterior_device(h, torch.from_numpy(np.ascontiguousarray(y)).to("cuda:0"))
    torch.cuda.synchronize()
    return img.cpu().numpy()


# ---- the image against NumPy -------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["float32", "float64"])
@pytest.mark.parametrize("T", [1, 17])
@pytest.mark.parametrize("V", [1, 63, 65, 257])
def test_image_is_build_initial_mvn_at_the_edges_of_the_grid(library, V, T, f64):
    """white noise with one precision; invrec_init with an image prior on T1 (the LOG row differs from voxel to voxel),
    multiexp_init with its defaults"""
    y = series(V, T, f64, seed=1000 + 10 * V + T)
    t1 = np.random.default_rng(V).uniform(0.5, 2.0, V)
    h = invrec_config(V, T, param_overrides={"T1": dict(type="I")}, image_priors={"T1": t1})
    assert hiplib.init_posterior_kernel_name(h) == "init<invrec_init>"
    want, logs = numpy_image(h, y, "invrec")
    assert_image(device_image(h, y), want, logs, "invrec_init V=%d T=%d" % (V, T))
    if V >= 63:  # the voxel of zeros kept the default M0; the NaN sample was skipped (T = 1: nothing else, the default)
        nCov = 4 * 5 // 2
        assert want[nCov, 3] == 1.0 and want[nCov, 5] == (np.nanmax(np.abs(y[:, 5].astype(np.float64))) if T > 1 else 1.0)
    h = multiexp_config(V, T)
    want, logs = numpy_image(h, y, "multiexp")
    assert_image(device_image(h, y), want, logs, "multiexp_init V=%d T=%d" % (V, T))


def test_host_pointers_give_the_bits_of_the_device_entry_point(library):
    y = series(257, 17, False, seed=11)
    t1 = np.random.default_rng(12).uniform(0.5, 2.0, 257)
    h = invrec_config(257, 17, param_overrides={"T1": dict(type="I")}, image_priors={"T1": t1})
    assert np.array_equal(hiplib.init_posterior_host(h, y), device_image(h, y), equal_nan=True)


NOISE_CASES = {
    "pattern 123": (17, dict(noise_pattern="123")),
    "ar1 one echo": (17, dict(noise=vbabi.NOISE_AR1, num_echoes=1)),
    "ar1 two echoes, dual, given alphas": (18, dict(noise=vbabi.NOISE_AR1, num_echoes=2, ar_cross_terms="dual", ar_alpha_post=(
        np.array([0.1, -0.2, 0.05, 0.3]),
        np.array([[2.0, 0.25, 0.0, 0.0], [0.25, 3.0, 0.0, -0.5], [0.0, 0.0, 4.0, 0.0], [0.0, -0.5, 0.0, 5.0]])))),
}


@pytest.mark.parametrize("case", sorted(NOISE_CASES))
def test_noise_rows(library, case):
    T, opts = NOISE_CASES[case]
    V = 65
    y = series(V, T, False, seed=77)
    for model, h in (("invrec", invrec_config(V, T, **opts)), ("multiexp", multiexp_config(V, T, **opts))):
        want, logs = numpy_image(h, y, model)
        n = h.cfg.n_params + h.n_noise_outputs
        assert want.shape[0] == vbabi.mvn_rows(n)
        assert_image(device_image(h, y), want, logs, "%s %s" % (model, case))
    if "given" in case:  # (the off-diagonal entry of the given covariance is in the image)
        P, n = 2, 2 + 4 + 2
        assert want[(P + 1) * (P + 2) // 2 + P, 0] == 0.25 and want[(P + 3) * (P + 4) // 2 + P + 1, 0] == -0.5


def test_more_than_32_parameters_take_the_table(library):
    """17 exponentials: P = 34 - the entry values come from fvb_config.params_ext and the kernel is the instance for up
    to FVB_MAX_PARAMS_EXT parameters"""
    V, T = 3, 8
    y = series(V, T, False, seed=34)
    h = multiexp_config(V, T, num_exps=17, dt=0.1)
    assert h.cfg.n_params == 34 > vbabi.FVB_MAX_PARAMS and h.cfg.params_ext
    assert hiplib.init_posterior_kernel_name(h) == "init<multiexp_init>"
    want, logs = numpy_image(h, y, "multiexp")
    assert len(logs) == 2 * 17
    assert_image(device_image(h, y), want, logs, "multiexp_init with 17 exponentials")
    assert np.array_equal(hiplib.init_posterior_host(h, y), device_image(h, y), equal_nan=True)


# ---- the routes consume it ---------------------------------------------------------------------------------------
def multiexp_series(V, T=50, dt=0.04, seed=5, noise_sd=0.05):
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None] * dt
    return (rng.uniform(0.5, 1.5, V) * np.exp(-rng.uniform(0.5, 1.5, V) * t) + rng.normal(0, noise_sd, (T, V))).astype(np.float32)


def same_bits(a, b, keys=("mvn", "free_energy", "status", "iterations")):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.all(a["status"] == 0) and np.isfinite(a["mvn"]).all()


def both_ways(make, y, run):
    """run(holder) without init_mvn, then given the image of init_posterior_device"""
    h = make()
    assert not h.cfg.init_mvn and hiplib.init_posterior_kernel_name(h).startswith("init<")
    own = run(h)
    given = make(init_mvn=device_image(h, y))
    assert hiplib.init_posterior_kernel_name(given) == ""
    return own, run(given)


def test_wave_kernels(library):
    V = 5
    y, _ = invrec_series(V, seed=41)

    def make(**kw):
        return vbabi.build_config(vbabi.MODEL_PLUGIN, V, len(TIS), device_model="invrec_init", constants=TIS, params=INVREC_PARAMS,
                                  need_f=True, **kw)
    assert hiplib.kernel_name(make()) == "wave<invrec_init>"
    same_bits(*both_ways(make, y, lambda h: hiplib.run_host(h, y)))


LANE_CASES = {"lane": (dict(need_f=True), "lane<multiexp_init,2"),
              "lane_ar1": (dict(noise=vbabi.NOISE_AR1, num_echoes=1, need_f=True), "lane_ar1<multiexp_init,2"),
              "lane_phis": (dict(noise_pattern="12", need_f=True), "lane_phis<multiexp_init,2")}


@pytest.mark.parametrize("case", sorted(LANE_CASES))
def test_lane_kernels(library, case):
    V = 65
    opts, kernel = LANE_CASES[case]
    y = multiexp_series(V)
    with variant("lane"):
        assert hiplib.kernel_name(multiexp_config(V, 50, **opts)).startswith(kernel)
        same_bits(*both_ways(lambda **kw: multiexp_config(V, 50, **opts, **kw), y, lambda h: hiplib.run_host(h, y)))


def test_spatial_vb(library):
    coords = vbabi.grid_coords((4, 4, 2))
    V = coords.shape[1]
    y = multiexp_series(V, seed=6)
    sp = vbabi.SpatialHolder(coords)

    def make(**kw):
        return multiexp_config(V, 50, max_iterations=3, need_f=True, param_overrides={"amp1": dict(type="M")}, **kw)
    assert hiplib.spatial_kernel_name(make()) == "spatial<multiexp_init,2>"
    same_bits(*both_ways(make, y, lambda h: hiplib.run_spatial_host(h, sp, y)))


def test_device_pointers(library):
    """fabber_vb_run_device: series, outputs and constants in device memory"""
    import torch
    from fabber_core_amd.device import DeviceProblem
    V = 65
    y, _ = invrec_series(V, seed=42)

    def make(**kw):
        return vbabi.build_config(vbabi.MODEL_PLUGIN, V, len(TIS), device_model="invrec_init", constants=TIS, params=INVREC_PARAMS,
                                  need_f=True, **kw)

    def run(h):
        prob = DeviceProblem(h, y, "cuda:0")
        L = hiplib.lib()
        stream = torch.cuda.current_stream(prob.device)
        rc = L.fabber_vb_run_device(C.byref(prob.cfg), prob.data.data_ptr(), C.byref(prob.out), C.c_void_p(stream.cuda_stream))
        assert rc == 0, L.fabber_vb_last_error().decode()
        return prob.results()
    own, given = both_ways(make, y, run)
    same_bits(own, given)
    same_bits(own, hiplib.run_host(make(), y))


def test_host_entry_point_cut_into_blocks(library, monkeypatch):
    """every pipelined block initialises its own columns (its slot holds the image); and the several-blocks entry point
    with the one device listed twice"""
    V = 200
    y = multiexp_series(V, seed=7)

    def make(**kw):
        return multiexp_config(V, 50, need_f=True, **kw)
    with variant("lane"):
        monkeypatch.setenv("FVB_HOST_BLOCK_VOXELS", "0")
        one = hiplib.run_host(make(), y)
        monkeypatch.setenv("FVB_HOST_BLOCK_VOXELS", "64")
        own, given = both_ways(make, y, lambda h: hiplib.run_host(h, y))
        same_bits(own, given)
        same_bits(own, one)
        monkeypatch.setenv("FVB_HOST_BLOCK_VOXELS", "0")
        own, given = both_ways(make, y, lambda h: hiplib.run_host(h, y, devices=[0, 0]))
        same_bits(own, given)
        same_bits(own, one)


# ---- refusals ----------------------------------------------------------------------------------------------------
def test_a_body_without_an_init_entry_is_refused_as_before(library):
    V, T = 65, 17
    y = series(V, T, False, seed=8)
    h = multiexp_config(V, T, name="multiexp_noinit")
    assert hiplib.init_posterior_kernel_name(h) == ""
    with pytest.raises(hiplib.HipEngineError, match="-52.*host-evaluated models need the initial posterior as init_mvn "
                                                    "\\(the model's InitVoxelPosterior runs on the host\\)"):
        hiplib.run_host(h, y)
    with pytest.raises(hiplib.HipEngineError, match="-95.*'multiexp_noinit'.*FABBER_DEVICE_INIT_MODEL"):
        device_image(h, y)
    with pytest.raises(hiplib.HipEngineError, match="-95.*'multiexp_noinit'"):
        hiplib.init_posterior_host(h, y)
    sp = vbabi.SpatialHolder(vbabi.grid_coords((5, 13, 1)))
    with pytest.raises(hiplib.HipEngineError, match="-40"):  # (and no spatial kernels either: the refusal of before)
        hiplib.run_spatial_host(multiexp_config(V, T, name="multiexp_noinit", param_overrides={"amp1": dict(type="M")}), sp, y)


def test_a_built_in_model_is_refused(library):
    h = vbabi.build_config(vbabi.MODEL_EXP, 65, 17, num_exps=1, dt=0.04)
    y = series(65, 17, False, seed=9)
    with pytest.raises(hiplib.HipEngineError, match="-95.*built-in model"):
        device_image(h, y)


# ---- through fabber_dorun ----------------------------------------------------------------------------------------
SHAPE = (6, 5, 4)
INIT_LINE = "the initial posterior comes from the body '%s' of its library (kernel init<%s>)"
SAVE = {"save-mean": True, "save-mvn": True, "save-free-energy": True, "save-model-fit": True}


@pytest.fixture(scope="module")
def old_libraries():
    """the same host classes in libraries without an init entry: wave bodies only (multiexp_dev, invrec), and bodies with
    spatial kernels (multiexp_sp)"""
    return device_model_lib.build_library(), device_model_lib.build_spatial_library()


def multiexp_volume(seed, T=40, dt=0.04, noise_sd=0.2):
    rng = np.random.default_rng(seed)
    t = np.arange(T) * dt
    amp = np.where(rng.random(SHAPE) < 0.5, 1.0, 0.5)
    rate = np.where(rng.random(SHAPE) < 0.5, 1.0, 0.8)
    return (amp[..., None] * np.exp(-rate[..., None] * t) + rng.normal(0, noise_sd, SHAPE + (T,))).astype(np.float32)


def invrec_volume_and_options(model):
    y, _ = invrec_series(120, seed=31, noise_sd=2.0)  # (the data of test_invrec_device_route_against_its_host_route)
    opts = dict(SAVE, **{"model": model, "noise": "white", "max-iterations": 6})
    for i, ti in enumerate(TIS):
        opts["ti%d" % (i + 1)] = float(ti)
    return y.T.reshape(SHAPE + (len(TIS),)).copy(), opts


def test_invrec_init_under_vb(library, old_libraries):
    data, opts = invrec_volume_and_options("invrec_init")
    opts["method"] = "vb"
    new = fabber.run(data, opts, model_libs=[library])
    old = fabber.run(data, dict(opts, model="invrec"), model_libs=[old_libraries[0]])
    assert "kernel wave<invrec_init>" in new["log"] and INIT_LINE % ("invrec_init", "invrec_init") in new["log"]
    assert "kernel wave<invrec>" in old["log"] and "init<" not in old["log"]
    assert_routes_agree(new, old, ("mean_M0", "mean_T1", "mean_a"))
    assert np.allclose(old["modelfit"], new["modelfit"], rtol=2e-5, atol=2e-5 * float(np.abs(data).max()))
    # host-model: the model's host code throughout, and no such line
    host = fabber.run(data, dict(opts, **{"host-model": True}), model_libs=[library])
    assert "init<" not in host["log"] and "evaluated on the host" in host["log"]
    assert_routes_agree(new, host, ("mean_M0", "mean_T1", "mean_a"))


def test_invrec_init_under_spatial_vb_keeps_the_host_route(library, old_libraries):
    """this library has no spatial kernels for invrec_init: the fit falls back to the model's host code, which needs the
    image on the host - built there as before, with no word of the kernel in the log"""
    data, opts = invrec_volume_and_options("invrec_init")
    opts.update({"method": "spatialvb", "param-spatial-priors": "MNN", "max-iterations": 4})
    new = fabber.run(data, opts, model_libs=[library])
    old = fabber.run(data, dict(opts, model="invrec"), model_libs=[old_libraries[0]])
    assert "init<" not in new["log"] and "evaluated on the host" in new["log"]
    assert_routes_agree(new, old, ("mean_M0", "mean_T1", "mean_a"))


@pytest.mark.parametrize("method", ["vb", "spatialvb"])
def test_multiexp_init_through_fabber_run(library, old_libraries, method):
    data = multiexp_volume(seed=151)
    opts = dict(SAVE, **{"model": "multiexp_init", "num-exps": 1, "dt": 0.04, "noise": "white", "method": method, "max-iterations": 5})
    if method == "spatialvb":
        opts["param-spatial-priors"] = "MN"
        other, other_lib, kernel = "multiexp_sp", old_libraries[1], "kernels spatial<%s,2>"
    else:
        other, other_lib, kernel = "multiexp_dev", old_libraries[0], "kernel wave<%s>"
    with variant("wave" if method == "vb" else "auto"):  # (multiexp_dev has no lane kernels: the same kernels on both sides)
        new = fabber.run(data, opts, model_libs=[library])
        old = fabber.run(data, dict(opts, model=other), model_libs=[other_lib])
        host = fabber.run(data, dict(opts, **{"host-model": True}), model_libs=[library])
    assert kernel % "multiexp_init" in new["log"] and INIT_LINE % ("multiexp_init", "multiexp_init") in new["log"]
    assert kernel % other in old["log"] and "init<" not in old["log"]
    assert "init<" not in host["log"] and "evaluated on the host" in host["log"]
    assert_routes_agree(new, old, ("mean_amp1", "mean_r1"))
    assert np.allclose(old["modelfit"], new["modelfit"], rtol=2e-5, atol=1e-5)
    assert_routes_agree(new, host, ("mean_amp1", "mean_r1"))
