"""Forward models of a model library that bring their own device body (include/fabber_device_model.h): the library's
kernels - the engine's wave-per-voxel loop around the library's evaluator, in the library's code object - against the
CPU oracle, and the device route of fabber_dorun against the host-model route of the same library
(tests/plugins/fwdmodel_device_models.hip: multiexp_dev, invrec)."""
import re

import numpy as np
import pytest

import cases
import device_model_lib
import oracle
import parity
from fabber_core_amd import fabber, hiplib, vbabi

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]


@pytest.fixture(scope="module")
def library():
    assert hiplib.available() and hiplib.device_count() > 0
    path = device_model_lib.build_library()
    hiplib.load_model_library(path)
    assert {"multiexp_dev", "invrec"} <= set(hiplib.device_models())
    return path


# ---- multiexp_dev through the C ABI against the oracle's MODEL_EXP -----------------------------------------------
def initial_mvn(h, y):
    """the initial posterior image as Vb::BuildInitialMvn writes it, white or AR(1) noise: the exponential model's
    data-dependent means (hiplib.initial_mvn), the noise block of the noise model's initial posterior - AR(1): the
    alphas N(0, 1e4 I) first (noisemodel_ar.cc:379-403), then the precisions"""
    cfg = h.cfg
    if cfg.noise == vbabi.NOISE_WHITE:
        return hiplib.initial_mvn(h, y)
    P, NA, N, V = cfg.n_params, 2 + cfg.ar_cross_terms, cfg.n_phis, cfg.n_voxels
    white = vbabi.build_config(vbabi.MODEL_EXP, V, cfg.n_times, num_exps=P // 2, dt=cfg.model_dopt[0])
    w = hiplib.initial_mvn(white, y)
    nw, n = P + 1, P + NA + N
    img = np.zeros((vbabi.mvn_rows(n), V))
    nCov = n * (n + 1) // 2
    for i in range(P):
        img[i * (i + 1) // 2 + i] = w[i * (i + 1) // 2 + i]
        img[nCov + i] = w[nw * (nw + 1) // 2 + i]
    for a in range(NA):
        q = P + a
        img[q * (q + 1) // 2 + q] = 1e4
    for k in range(N):
        b, c = cfg.noise_post_b[k], cfg.noise_post_c[k]
        q = P + NA + k
        img[q * (q + 1) // 2 + q] = b * b * c
        img[nCov + q] = b * c
    img[-1] = 1.0
    return img


def exp_pair(V, T, num_exps, dt, seed, **opts):
    """the same problem twice: for the oracle as the built-in exponential model, for the engine as the library's body
    (same parameters, priors and initial posterior image)"""
    ref, y = cases.exp_problem(V, T, num_exps, dt, seed=seed, **opts)
    mvn = initial_mvn(ref, y)
    ref, _ = cases.exp_problem(V, T, num_exps, dt, seed=seed, init_mvn=mvn, **opts)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_dev", num_exps=num_exps, dt=dt, init_mvn=mvn,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **opts)
    return ref, dev, y


EXP_CASES = {
    "white": dict(),
    "white,F": dict(need_f=True),
    "pattern 12,F": dict(noise_pattern="12", need_f=True),
    "ar1 one echo": dict(noise=vbabi.NOISE_AR1, num_echoes=1),
    "ar1 one echo,F": dict(noise=vbabi.NOISE_AR1, num_echoes=1, need_f=True),
    "ar1 two echoes,F": dict(noise=vbabi.NOISE_AR1, num_echoes=2, ar_cross_terms="dual", need_f=True),
}


@pytest.mark.parametrize("case", sorted(EXP_CASES))
def test_multiexp_dev_against_the_oracle(library, case):
    """The body computes the expression of the built-in exponential model and the kernel around it is the wave kernel:
    held to the bounds tests/test_wave_kernel.py holds that kernel to (parity.strict at its base tolerances, no raised
    floor; means within 1e-6)."""
    ref, dev, y = exp_pair(963, 50, 1, 0.04, seed=20260102, max_iterations=10, **EXP_CASES[case])
    assert hiplib.kernel_name(dev) == "wave<multiexp_dev>"
    got = hiplib.run_host(dev, y)
    r = parity.strict(ref, oracle.run(ref, y), got, what="multiexp_dev " + case, cpu2=oracle.run_fma(ref, y))
    print("multiexp_dev %s: err means %.3e cov %.3e F %.3e" % (case, r["err_means"], r["err_cov"], r["err_f"]))
    assert not r["raised"]
    assert r["err_means"] < 1e-6


def test_device_pointers_take_the_constants_like_the_design(library):
    """DeviceProblem uploads the constants block; the device entry point against the host entry point, bit for bit"""
    from fabber_core_amd.device import DeviceProblem
    h, y, _ = invrec_problem(256, seed=5)
    host = hiplib.run_host(h, y)
    prob = DeviceProblem(h, y, "cuda:0")
    assert prob.kernel == "wave<invrec>"
    prob.run()
    dev = prob.results()
    assert np.array_equal(host["mvn"], dev["mvn"]) and np.array_equal(host["status"], dev["status"])
    assert np.all(host["status"] == 0)


def test_plugin_model_needs_the_initial_posterior(library):
    h = vbabi.build_config(vbabi.MODEL_PLUGIN, 64, 16, device_model="invrec", constants=TIS, params=INVREC_PARAMS)
    with pytest.raises(hiplib.HipEngineError, match="-52.*init_mvn"):
        hiplib.run_host(h, np.zeros((16, 64), dtype=np.float32))


def test_other_entry_points_refuse_a_library_body(library):
    """method=nlls and spatial VB have no kernels for a library's body: the codes and messages of a model without kernels"""
    h, y, _ = invrec_problem(64, seed=6)
    with pytest.raises(hiplib.HipEngineError, match="-61.*device body"):
        hiplib.nlls_run_host(h, y)
    sp = vbabi.SpatialHolder(vbabi.grid_coords((4, 4, 4)))
    with pytest.raises(hiplib.HipEngineError, match="-40.*no spatial kernel"):
        hiplib.run_spatial_host(h, sp, y)


# ---- more than one block -----------------------------------------------------------------------------------------
def test_blocks_of_the_host_entry_point_are_the_run_in_one(library, monkeypatch):
    """fabber_vb_run_host pipelines blocks of voxels (upload, fit, download): every block gets the constants, every
    output identical to the run in one block"""
    h, y, _ = invrec_problem(1500, seed=7, need_f=True)
    monkeypatch.setenv("FVB_HOST_BLOCK_VOXELS", "0")
    one = hiplib.run_host(h, y)
    monkeypatch.setenv("FVB_HOST_BLOCK_VOXELS", "256")
    many = hiplib.run_host(h, y)
    for k in ("mvn", "free_energy", "status", "iterations"):
        assert np.array_equal(one[k], many[k]), k
    assert np.all(one["status"] == 0)
    if hiplib.device_count() >= 1:  # the same through the several-blocks entry point (one device listed twice)
        multi = hiplib.run_host(h, y, devices=[0, 0])
        assert np.array_equal(one["mvn"], multi["mvn"])


# ---- invrec ----------------------------------------------------------------------------------------------------------
TIS = np.linspace(0.1, 4.0, 16)
INVREC_PARAMS = [dict(name="M0", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
                 dict(name="T1", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG),
                 dict(name="a", prior=(0.8, 4.0), post=(0.8, 1.0), prior_type="N", transform=vbabi.TRANSFORM_FRACTIONAL)]


def invrec_series(V, seed, noise_sd=0.5):
    rng = np.random.default_rng(seed)
    truth = dict(M0=rng.uniform(80, 120, V), T1=rng.uniform(0.8, 1.6, V), a=rng.uniform(0.85, 0.98, V))
    y = truth["M0"] * (1 - 2 * truth["a"] * np.exp(-TIS[:, None] / truth["T1"]))
    return (y + rng.normal(0, noise_sd, y.shape)).astype(np.float32), truth


def invrec_problem(V, seed, **opts):
    """through the C ABI: the initial posterior as the library's InitVoxelPosterior sets it (M0 = max |y|)"""
    y, truth = invrec_series(V, seed)
    h = vbabi.build_config(vbabi.MODEL_PLUGIN, V, len(TIS), device_model="invrec", constants=TIS, params=INVREC_PARAMS, **opts)
    mvn = hiplib.initial_mvn(h, y)
    n = 4
    mvn[n * (n + 1) // 2 + 0] = np.abs(y.astype(np.float64)).max(axis=0)
    h = vbabi.build_config(vbabi.MODEL_PLUGIN, V, len(TIS), device_model="invrec", constants=TIS, params=INVREC_PARAMS, init_mvn=mvn, **opts)
    return h, y, truth


def invrec_options(**extra):
    opts = {"model": "invrec", "noise": "white", "method": "vb", "max-iterations": 6, "save-mean": True, "save-mvn": True,
            "save-free-energy": True, "save-model-fit": True, "save-residuals": True}
    for i, ti in enumerate(TIS):
        opts["ti%d" % (i + 1)] = float(ti)
    opts.update(extra)
    return opts


def both_routes(library, data, opts):
    dev = fabber.run(data, opts, model_libs=[library])
    host = fabber.run(data, dict(opts, **{"host-model": True}), model_libs=[library])
    assert "with the body '%s' of its library" % opts["model"] in dev["log"]
    assert "kernel wave<%s>" % opts["model"] in dev["log"]
    assert "evaluated on the host" in host["log"] and "of its library" not in host["log"]
    return dev, host


def assert_routes_agree(dev, host, means):
    """the tolerances tests/test_hostmodel.py applies to a host-evaluated copy of a built-in model (device exp against
    libm); every voxel. The free energy is compared RELATIVELY (rtol 1e-5, numpy's default atol of 1e-8), which only
    means something where F stays away from zero: F is a sum of terms of order T log(2 pi sigma^2) / 2 - tens - that can
    cancel. On the exponential problem below with a noise level of 0.05 the oracle's F runs from -1.5 to 5.9 through
    zero, and its two CPU builds (with and without FMA contraction) already differ by 2.1e-5 relative there (4.5e-6
    absolute); with 0.2 it runs from -27 to -9 and they differ by 1.5e-7 (AR(1): -87 to -71, 2e-10). So the problems
    here are given noise levels at which |F| > 1 everywhere, and that is asserted first."""
    assert np.abs(host["freeEnergy"]).min() > 1.0, "F passes near zero: the relative comparison of F is ill-posed on this data"
    for k in means:
        print("%s: max |dev - host| %.3e" % (k, np.max(np.abs(dev[k] - host[k]))))
        assert np.allclose(host[k], dev[k], rtol=2e-5, atol=1e-5), k
    assert np.allclose(host["finalMVN"], dev["finalMVN"], rtol=1e-4, atol=1e-7)
    assert np.allclose(host["freeEnergy"], dev["freeEnergy"], rtol=1e-5)


@pytest.mark.parametrize("noise", ["white", "ar"])
def test_multiexp_dev_device_route_against_its_host_route(library, noise):
    rng = np.random.default_rng(21)
    shape, T = (6, 5, 4), 40
    t = np.arange(T) * 0.04
    amp = np.where(rng.random(shape) < 0.5, 1.0, 0.5)
    rate = np.where(rng.random(shape) < 0.5, 1.0, 0.8)
    data = (amp[..., None] * np.exp(-rate[..., None] * t) + rng.normal(0, 0.2, shape + (T,))).astype(np.float32)
    opts = {"model": "multiexp_dev", "num-exps": 1, "dt": 0.04, "noise": noise, "method": "vb", "max-iterations": 5, "save-mean": True,
            "save-mvn": True, "save-free-energy": True, "save-model-fit": True}
    dev, host = both_routes(library, data, opts)
    assert_routes_agree(dev, host, ("mean_amp1", "mean_r1"))
    assert np.allclose(host["modelfit"], dev["modelfit"], rtol=2e-5, atol=1e-5)


def test_invrec_device_route_against_its_host_route(library):
    y, _ = invrec_series(120, seed=31, noise_sd=2.0)  # (a signal of order 100; F of order -40, see assert_routes_agree)
    data = y.T.reshape(6, 5, 4, len(TIS)).copy()
    dev, host = both_routes(library, data, invrec_options())
    assert_routes_agree(dev, host, ("mean_M0", "mean_T1", "mean_a"))
    # (both fits come from the host code, evaluated at means that agree to rtol 2e-5: on a curve of amplitude M0 that
    # passes through zero this is an absolute 2e-5 M0)
    assert np.allclose(host["modelfit"], dev["modelfit"], rtol=2e-5, atol=2e-5 * float(np.abs(data).max()))
    assert np.allclose(dev["modelfit"] + dev["residuals"], data, rtol=0, atol=1e-4)


def test_invrec_recovers_its_parameters(library):
    """M0, T1 and the inversion efficiency come back to the accuracy the host route reaches on the same data: both
    routes run the same updates on the same linearisation (they differ by the device's exp against libm, 1e-5 relative
    at the tolerances above), so the device route's error against the truth may exceed the host route's by that much"""
    V = 240
    y, truth = invrec_series(V, seed=32, noise_sd=0.2)
    data = y.T.reshape(8, 6, 5, len(TIS)).copy()
    dev, host = both_routes(library, data, invrec_options(**{"max-iterations": 12}))
    for name in ("M0", "T1", "a"):
        want = truth[name].reshape(8, 6, 5)
        e_dev = np.abs(dev["mean_" + name] - want) / np.abs(want)
        e_host = np.abs(host["mean_" + name] - want) / np.abs(want)
        print("invrec %s: relative error against the truth, device median %.3e max %.3e, host median %.3e max %.3e"
              % (name, np.median(e_dev), e_dev.max(), np.median(e_host), e_host.max()))
        # (rtol 2e-5, atol 1e-5 between the routes' means, as a relative error against the truth)
        assert np.all(e_dev <= e_host + 2e-5 * (1 + e_host) + 1e-5 / np.abs(want)), name
        assert np.median(e_dev) < 0.02, name  # (and the fit is a fit: noise of 0.2 on a signal of order 100)


def test_wrong_number_of_inversion_times_fails_cleanly_on_both_routes(library):
    """15 inversion times for 16 timepoints: the host code's EvaluateModel throws; on the device route nothing calls it
    before the kernel runs, so the body itself answers a timepoint without a constant with a non-finite prediction
    (never a read past the constants block) and the run stops on the non-finite offset of the set-up re-centre"""
    y, _ = invrec_series(24, seed=34)
    data = y.T.reshape(4, 3, 2, len(TIS)).copy()
    opts = invrec_options()
    del opts["ti%d" % len(TIS)]
    with pytest.raises(fabber.FabberError, match="Non-finite values found in offset"):
        fabber.run(data, opts, model_libs=[library])
    with pytest.raises(fabber.FabberError):
        fabber.run(data, dict(opts, **{"host-model": True}), model_libs=[library])
    # the same through the C ABI: every voxel stops in its set-up with the non-finite-offset status
    h, y2, _ = invrec_problem(64, seed=35)
    short = vbabi.build_config(vbabi.MODEL_PLUGIN, 64, len(TIS), device_model="invrec", constants=TIS[:-1], params=INVREC_PARAMS,
                               init_mvn=h.keep["init_mvn"])
    r = hiplib.run_host(short, y2)
    assert np.all(r["status"] == vbabi.STATUS_BAD_OFFSET) and np.all(r["setup_failed"])


# ---- what the device body does not serve -------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["spatialvb", "nlls"])
def test_unsupported_methods_fall_back_to_the_host_route(library, method):
    y, _ = invrec_series(120, seed=33)
    data = y.T.reshape(6, 5, 4, len(TIS)).copy()
    opts = invrec_options(method=method)
    if method == "spatialvb":
        opts.update({"param-spatial-priors": "MNN", "max-iterations": 3})
    for k in ("save-free-energy", "save-model-fit", "save-residuals"):
        opts.pop(k)
    out = fabber.run(data, opts, model_libs=[library])
    assert re.search("evaluated on the host", out["log"], re.I)
    assert "of its library" not in out["log"]
    if method == "spatialvb":
        assert "no device kernels for spatial VB" in out["log"]
    forced = fabber.run(data, dict(opts, **{"host-model": True}), model_libs=[library])
    assert np.array_equal(out["finalMVN"], forced["finalMVN"])


def test_a_failing_voxel_has_the_status_of_the_host_route(library):
    """a non-finite sample: the run fails unless bad voxels are allowed, and then that voxel - and only it - is reported
    with the reason the host route gives"""
    rng = np.random.default_rng(41)
    shape, T = (5, 4, 3), 40
    t = np.arange(T) * 0.04
    data = (np.exp(-t) + rng.normal(0, 0.05, shape + (T,))).astype(np.float32)
    data[1, 1, 1, 5] = np.nan
    opts = {"model": "multiexp_dev", "num-exps": 1, "dt": 0.04, "noise": "white", "method": "vb", "max-iterations": 5, "save-mean": True,
            "save-free-energy": True}
    with pytest.raises(fabber.FabberError):
        fabber.run(data, opts, model_libs=[library])
    dev, host = both_routes(library, data, dict(opts, **{"allow-bad-voxels": True}))
    bad = lambda log: [l.strip() for l in log.splitlines() if "Internal error for voxel" in l or "numerical errors" in l]
    assert bad(dev["log"]) and bad(dev["log"]) == bad(host["log"])
    assert len([l for l in bad(dev["log"]) if "Internal error for voxel" in l]) == 1
    sel = np.ones(shape, dtype=bool)
    sel[1, 1, 1] = False
    assert np.allclose(host["mean_amp1"][sel], dev["mean_amp1"][sel], rtol=2e-5, atol=1e-5)
