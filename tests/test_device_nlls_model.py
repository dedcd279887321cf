"""method=nlls around the device body of a model library (include/fabber_device_nlls_model.h): the engine's wave-per-voxel
and lane-per-voxel minimisers compiled in the library's code object around the library's evaluator
(tests/plugins/fwdmodel_nlls_models.hip: multiexp_nlls, invrec_nlls) - against the CPU oracle's run of the built-in
exponential model, against SciPy's least-squares solution, lane against wave, and through fabber_dorun against the
host-model route of the same library. The bounds are those of tests/test_nlls.py.

The shapes are the smallest at which these kernels can go wrong: 2048 voxels as tests/test_nlls.py, 4200 for the
automatic choice of the lane minimiser (past the 4096 of the size rule, not a multiple of the 64 voxels of a wavefront),
300 and 130 voxels for partial wavefronts."""
import contextlib

import numpy as np
import pytest
import scipy.optimize

import cases
import device_model_lib
import oracle
from fabber_core_amd import fabber, hiplib, vbabi

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]

ENTRIES = {("multiexp_nlls", 0), ("multiexp_nlls", 2), ("multiexp_nlls", 4), ("invrec_nlls", 0), ("invrec_nlls", 3)}


@pytest.fixture(scope="module")
def library():
    assert hiplib.available() and hiplib.device_count() > 0
    path = device_model_lib.build_nlls_library()
    hiplib.load_model_library(path)
    assert ENTRIES <= set(hiplib.device_nlls_models())
    return path


@contextlib.contextmanager
def variant(name):
    hiplib.set_variant(name)
    try:
        yield
    finally:
        hiplib.set_variant("auto")


def run_variant(name, h, y, **kw):
    with variant(name):
        kernel = hiplib.nlls_kernel_name(h)
        res = hiplib.nlls_run_host(h, y, **kw)
    return kernel, res


# ---- multiexp_nlls through the C ABI against the oracle's MODEL_EXP --------------------------------------------------
def exp_pair(V, T, seed, **opts):
    """the same problem twice: for the oracle as the built-in exponential model, for the library's minimisers as its body
    (the same parameters and transforms)"""
    ref, y = cases.exp_problem(V, T, 1, 0.04, seed=seed, **opts)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_nlls", num_exps=1, dt=0.04,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1), **opts)
    return ref, dev, y


_ORACLE = {}


def oracle_once(key, ref, y, **kw):
    """the oracle's result of a problem, computed once for the tests that share it (and left unchanged)"""
    if key not in _ORACLE:
        _ORACLE[key] = oracle.run_nlls(ref, y, **kw)
    return _ORACLE[key]


def assert_parity_bounds(ref, got, P, what, tol=1e-4):
    """the bounds of assert_parity in tests/test_nlls.py: status arrays equal; means within 1e-4 of max(|mean|, sd) for
    every voxel and within 1e-6 for 99 % of them; cost rtol 1e-7; covariance entries, against the scale of their row and
    column, 1e-3 at the maximum and 1e-5 at the 99 % quantile. The number of iterations is not compared (see there)."""
    assert np.array_equal(ref["status"], got["status"])
    ok = ref["status"] == 0
    off = P * (P + 1) // 2
    sd = np.sqrt(np.abs(np.stack([ref["mvn"][p * (p + 1) // 2 + p] for p in range(P)])))
    scale = np.maximum(np.abs(ref["mvn"][off:off + P]), sd)
    err = (np.abs(got["mvn"][off:off + P] - ref["mvn"][off:off + P]) / np.maximum(scale, 1e-300))[:, ok]
    cost = np.max(np.abs(got["cost"][ok] - ref["cost"][ok]) / np.abs(ref["cost"][ok]))
    cov = []
    row = 0
    for r in range(P):
        for c in range(r + 1):
            cov.append(np.abs(got["mvn"][row] - ref["mvn"][row])[ok] / (sd[r] * sd[c])[ok])
            row += 1
    print("%s: means max %.3e q99 %.3e; cost max relative %.3e; covariance max %.3e q99 %.3e"
          % (what, err.max(), np.quantile(err.max(axis=0), 0.99), cost, max(d.max() for d in cov), max(np.quantile(d, 0.99) for d in cov)))
    assert err.max() < tol, err.max()
    assert np.quantile(err.max(axis=0), 0.99) < 1e-6, np.quantile(err.max(axis=0), 0.99)
    assert np.allclose(got["cost"][ok], ref["cost"][ok], rtol=1e-7, atol=1e-12)
    for d in cov:
        assert d.max() < 1e-3 and np.quantile(d, 0.99) < 1e-5, d.max()


@pytest.mark.parametrize("name", ["lane", "wave"])
@pytest.mark.parametrize("lm", [False, True])
def test_multiexp_against_the_oracle(library, lm, name):
    ref, dev, y = exp_pair(2048, 50, seed=20260102)
    kernel, got = run_variant(name, dev, y, lm=lm)
    assert kernel == {"lane": "nlls<multiexp_nlls,2>", "wave": "nlls_wave<multiexp_nlls>"}[name]
    assert_parity_bounds(oracle_once(("exp", lm), ref, y, lm=lm), got, 2, "%s lm=%s" % (kernel, lm))


def test_multiexp_takes_the_lane_minimiser_by_the_size_rule(library):
    """4200 voxels: 65 full wavefronts and 40 lanes of the last one"""
    ref, dev, y = exp_pair(4200, 50, seed=20260105)
    assert hiplib.nlls_kernel_name(dev) == "nlls<multiexp_nlls,2>"
    got = hiplib.nlls_run_host(dev, y)
    assert_parity_bounds(oracle.run_nlls(ref, y), got, 2, "nlls<multiexp_nlls,2> 4200 voxels")


@pytest.mark.parametrize("name", ["lane", "wave"])
def test_multiexp_with_masked_timepoints(library, name):
    ref, dev, y = exp_pair(300, 40, seed=20260106, masked_timepoints=(5, 17))
    kernel, got = run_variant(name, dev, y)
    assert kernel.startswith("nlls<multiexp_nlls,2>" if name == "lane" else "nlls_wave<multiexp_nlls>")
    expect = oracle_once("masked", ref, y)
    assert_parity_bounds(expect, got, 2, kernel + " masked timepoints")
    unmasked, _, _ = exp_pair(300, 40, seed=20260106)
    assert not np.allclose(oracle_once("unmasked", unmasked, y)["mvn"][3], expect["mvn"][3], rtol=1e-9)  # (the mask matters)


# ---- invrec_nlls: constants block, LOG and FRACTIONAL transforms ------------------------------------------------------
TIS = np.linspace(0.1, 3.0, 12)
INVREC_PARAMS = [dict(name="M0", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
                 dict(name="T1", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG),
                 dict(name="a", prior=(0.8, 4.0), post=(0.8, 1.0), prior_type="N", transform=vbabi.TRANSFORM_FRACTIONAL)]
# Fabber space, near the truth of every voxel of invrec_series: M0 = 100, T1 = 1.2, a = 0.9
INVREC_START = [100.0, np.log(1.2), vbabi.to_fabber(vbabi.TRANSFORM_FRACTIONAL, 0.9)]
INVREC_SEED = 61


def invrec_series(V, seed, noise_sd=0.5):
    """a signal of order 100 with noise of 0.5; the truth stays near INVREC_START, so that every voxel has one basin
    (checked with SciPy from the start, from the truth and from perturbed starts for the seeds used here)"""
    rng = np.random.default_rng(seed)
    truth = dict(M0=rng.uniform(90, 110, V), T1=rng.uniform(1.0, 1.4, V), a=rng.uniform(0.87, 0.93, V))
    clean = truth["M0"] * (1 - 2 * truth["a"] * np.exp(-TIS[:, None] / truth["T1"]))
    return (clean + rng.normal(0, noise_sd, clean.shape)).astype(np.float32), truth


def invrec_config(V, name="invrec_nlls", constants=TIS):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, len(TIS), device_model=name, constants=constants, params=INVREC_PARAMS)


def invrec_residual(q, y):
    """the model in Fabber space (fwdmodel.cc:375-379: LOG and FRACTIONAL transforms) minus the series"""
    return q[0] * (1 - 2 * (1 / (1 + np.exp(q[2]))) * np.exp(-TIS / np.exp(q[1]))) - y


def scipy_fit(y, start=INVREC_START):
    return scipy.optimize.least_squares(invrec_residual, start, args=(y.astype(np.float64),), xtol=1e-14, ftol=1e-14, gtol=1e-14)


def covariance(res, P, v):
    cov = np.zeros((P, P))
    row = 0
    for r in range(P):
        for c in range(r + 1):
            cov[r, c] = cov[c, r] = res["mvn"][row, v]
            row += 1
    return cov


@pytest.mark.parametrize("name", ["lane", "wave"])
def test_invrec_matches_scipy_least_squares(library, name):
    """Means = the least-squares solution; covariance = mse (J'J)^-1 (inference_nlls.cc:160-173): the bounds of
    test_exponential_fit_matches_scipy_least_squares, the means within 1e-4 of max(|mean|, sd)."""
    V, P, T = 16, 3, len(TIS)
    y, _ = invrec_series(V, INVREC_SEED)
    h = invrec_config(V)
    kernel, res = run_variant(name, h, y, start=INVREC_START)
    assert kernel == {"lane": "nlls<invrec_nlls,3>", "wave": "nlls_wave<invrec_nlls>"}[name]
    assert np.all(res["status"] == 0)
    theta = res["mvn"][6:9]
    worst = dict(mean=0.0, cost=0.0, cov=0.0)
    sols = [scipy_fit(y[:, v]) for v in range(V)]
    for v, sol in enumerate(sols):
        expect = np.linalg.inv(sol.jac.T @ sol.jac) * (2 * sol.cost / (T - P))
        scale = np.maximum(np.abs(sol.x), np.sqrt(np.diag(expect)))
        worst["mean"] = max(worst["mean"], np.max(np.abs(theta[:, v] - sol.x) / scale))
        worst["cost"] = max(worst["cost"], abs(res["cost"][v] / (2 * sol.cost) - 1))
        worst["cov"] = max(worst["cov"], np.max(np.abs(covariance(res, P, v) / expect - 1)))
    print("%s against SciPy: means %.3e of max(|mean|, sd); cost relative %.3e; covariance relative %.3e"
          % (kernel, worst["mean"], worst["cost"], worst["cov"]))
    for v, sol in enumerate(sols):
        expect = np.linalg.inv(sol.jac.T @ sol.jac) * (2 * sol.cost / (T - P))
        scale = np.maximum(np.abs(sol.x), np.sqrt(np.diag(expect)))
        assert np.all(np.abs(theta[:, v] - sol.x) <= 1e-4 * scale), (v, theta[:, v], sol.x)
        assert np.isclose(res["cost"][v], 2 * sol.cost, rtol=1e-8)
        assert np.allclose(covariance(res, P, v), expect, rtol=2e-3), (v, covariance(res, P, v), expect)


def test_invrec_lane_against_wave(library):
    """130 voxels: two full wavefronts and two lanes"""
    V, P = 130, 3
    y, _ = invrec_series(V, INVREC_SEED + 1)
    h = invrec_config(V)
    _, lane = run_variant("lane", h, y, start=INVREC_START)
    _, wave = run_variant("wave", h, y, start=INVREC_START)
    assert np.array_equal(lane["status"], wave["status"]) and np.all(wave["status"] == 0)
    sd = np.sqrt(np.stack([wave["mvn"][p * (p + 1) // 2 + p] for p in range(P)]))
    scale = np.maximum(np.abs(wave["mvn"][6:9]), sd)
    err = np.abs(lane["mvn"][6:9] - wave["mvn"][6:9]) / scale
    print("nlls<invrec_nlls,3> against nlls_wave<invrec_nlls>: means %.3e of max(|mean|, sd)" % err.max())
    assert err.max() <= 1e-4


def test_too_few_constants_give_every_voxel_the_uninformative_precision(library):
    """11 inversion times for 12 timepoints: the body answers the timepoint without a constant with a non-finite
    prediction - nothing is read past the constants block - and every voxel takes the catch branch of
    inference_nlls.cc:186-207: the start as its means, precisions 1e-12 I"""
    V = 70
    y, _ = invrec_series(V, INVREC_SEED + 2)
    short = invrec_config(V, constants=TIS[:-1])
    results = {}
    for name in ("lane", "wave"):
        _, r = run_variant(name, short, y, start=INVREC_START)
        assert np.all(r["status"] != 0)
        for row, want in zip(range(6), (1e12, 0.0, 1e12, 0.0, 0.0, 1e12)):
            assert np.all(r["mvn"][row] == want), (name, row)
        for i in range(3):
            assert np.all(r["mvn"][6 + i] == INVREC_START[i]), (name, i)
        assert np.all(r["mvn"][9] == 1.0)
        results[name] = r
    assert np.array_equal(results["lane"]["mvn"], results["wave"]["mvn"])
    assert np.array_equal(results["lane"]["status"], results["wave"]["status"])


def test_non_finite_exponential_is_the_oracle_bit_for_bit(library):
    """test_non_finite_model_on_the_gpu of tests/test_nlls.py with the library's body: exp(+1e6 t) overflows"""
    ref, dev, y = exp_pair(70, 20, seed=1)
    ref.cfg.transform[1] = dev.cfg.transform[1] = vbabi.TRANSFORM_IDENTITY
    expect = oracle.run_nlls(ref, y, start=[0.0, -1e6])
    assert np.all(expect["status"] != 0)
    for name in ("lane", "wave"):
        _, got = run_variant(name, dev, y, start=[0.0, -1e6])
        assert np.array_equal(expect["status"] != 0, got["status"] != 0)
        assert np.array_equal(expect["mvn"], got["mvn"])


# ---- through fabber_dorun ------------------------------------------------------------------------------------------------
SHAPE = (6, 5, 4)


def both_routes(library, data, opts):
    dev = fabber.run(data, opts, model_libs=[library])
    host = fabber.run(data, dict(opts, **{"host-model": True}), model_libs=[library])
    assert "with the body '%s' of its library" % opts["model"] in dev["log"]
    assert "kernel nlls_wave<%s>" % opts["model"] in dev["log"]  # (120 voxels: the wave minimiser)
    assert "evaluated on the host" in host["log"] and "of its library" not in host["log"]
    return dev, host


def assert_routes_agree(dev, host, means):
    """assert_routes_agree of tests/test_device_model.py without the free energy, which NLLS does not have"""
    for k in means:
        print("%s: max |dev - host| %.3e" % (k, np.nanmax(np.abs(dev[k] - host[k]))))
        assert np.allclose(host[k], dev[k], rtol=2e-5, atol=1e-5, equal_nan=True), k
    assert np.allclose(host["finalMVN"], dev["finalMVN"], rtol=1e-4, atol=1e-7, equal_nan=True)


def test_multiexp_through_fabber_run_against_the_host_model_route(library):
    rng = np.random.default_rng(71)
    T = 40
    t = np.arange(T) * 0.04
    amp = np.where(rng.random(SHAPE) < 0.5, 1.0, 0.5)
    rate = np.where(rng.random(SHAPE) < 0.5, 1.0, 0.8)
    data = (amp[..., None] * np.exp(-rate[..., None] * t) + rng.normal(0, 0.05, SHAPE + (T,))).astype(np.float32)
    opts = {"model": "multiexp_nlls", "num-exps": 1, "dt": 0.04, "noise": "white", "method": "nlls", "save-mean": True, "save-mvn": True,
            "save-model-fit": True, "save-residuals": True}
    dev, host = both_routes(library, data, opts)
    assert_routes_agree(dev, host, ("mean_amp1", "mean_r1"))
    assert np.allclose(dev["mean_amp1"], amp, atol=0.2) and np.allclose(dev["mean_r1"], rate, atol=0.3)  # (the fit is a fit)
    assert np.allclose(dev["modelfit"] + dev["residuals"], data, rtol=0, atol=1e-4)
    assert np.allclose(host["modelfit"], dev["modelfit"], rtol=2e-5, atol=1e-5)


def test_invrec_through_fabber_run_honours_the_starting_estimate_on_both_routes(library, tmp_path):
    """fwd-inital-posterior gives the starting estimate (inference_nlls.cc:68-82) on both routes: the fits agree, and a voxel
    with a non-finite sample - every cost comparison is false there, the minimiser gives up at once - comes back with
    exactly that start"""
    y, truth = invrec_series(120, INVREC_SEED + 3)
    data = y.T.reshape(SHAPE + (len(TIS),)).copy()
    data[1, 1, 1, 4] = np.nan
    rest = np.ones(SHAPE, dtype=bool)
    rest[1, 1, 1] = False
    start = np.zeros((4, 4))
    start[:3, :3] = np.eye(3)
    start[:3, 3] = start[3, :3] = INVREC_START
    start[3, 3] = 1.0
    np.savetxt(str(tmp_path / "start.mat"), start)
    opts = {"model": "invrec_nlls", "noise": "white", "method": "nlls", "save-mean": True, "save-mvn": True, "save-model-fit": True,
            "save-residuals": True, "fwd-inital-posterior": str(tmp_path / "start.mat")}
    for i, ti in enumerate(TIS):
        opts["ti%d" % (i + 1)] = float(ti)
    dev, host = both_routes(library, data, opts)
    assert_routes_agree(dev, host, ("mean_M0", "mean_T1", "mean_a"))
    for out in (dev, host):
        assert out["mean_M0"][1, 1, 1] == np.float32(100.0)
        assert np.isclose(out["mean_T1"][1, 1, 1], 1.2, rtol=1e-6) and np.isclose(out["mean_a"][1, 1, 1], 0.9, rtol=1e-6)
        assert out["finalMVN"][1, 1, 1, 0] == np.float32(1e12)
    # (the model's own starting estimate, which the file replaces, has M0 = 1)
    assert np.allclose(dev["mean_M0"][rest], truth["M0"].reshape(SHAPE)[rest], rtol=0.05)
    assert np.allclose((dev["modelfit"] + dev["residuals"])[rest], data[rest], rtol=0, atol=1e-4)


# ---- a library without the new macros --------------------------------------------------------------------------------------
def test_a_library_without_nlls_entries_keeps_the_host_route(library):
    """tests/plugins/fwdmodel_device_models.hip (wave VB bodies only), loaded next to the NLLS library: method=nlls for
    its invrec is evaluated on the host and the C ABI refuses the body, as before"""
    old = device_model_lib.build_library()
    hiplib.load_model_library(old)
    y, _ = invrec_series(120, INVREC_SEED + 4)
    data = y.T.reshape(SHAPE + (len(TIS),)).copy()
    opts = {"model": "invrec", "noise": "white", "method": "nlls", "save-mean": True, "save-mvn": True}
    for i, ti in enumerate(TIS):
        opts["ti%d" % (i + 1)] = float(ti)
    out = fabber.run(data, opts, model_libs=[old])
    assert "evaluated on the host" in out["log"] and "of its library" not in out["log"] and "kernel nlls" not in out["log"]
    h = invrec_config(120, name="invrec")
    assert hiplib.nlls_kernel_name(h) == ""
    with pytest.raises(hiplib.HipEngineError, match="-61.*device body"):
        hiplib.nlls_run_host(h, y, start=INVREC_START)
