"""Lane-per-voxel kernels around the device body of a model library (include/fabber_device_lane_model.h): the engine's
lane kernel compiled in the library's code object around the library's evaluator, against the CPU oracle, against the
wave-per-voxel kernels of the same body, and through fabber_dorun against the host-model route of the same library
(tests/plugins/fwdmodel_lane_models.hip: multiexp_lane, invrec_lane).

The shapes are the smallest at which this kernel can go wrong: 197 voxels are three full wavefronts and five lanes, 21
timepoints are neither a multiple of the 8-timepoint trip nor of the 4-sample tile group; the `lane` variant forces the
kernel at these sizes."""
import contextlib

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
    path = device_model_lib.build_lane_library()
    hiplib.load_model_library(path)
    assert {("multiexp_lane", 2), ("multiexp_lane", 4), ("invrec_lane", 3)} <= set(hiplib.device_lane_models())
    return path


@contextlib.contextmanager
def variant(name):
    hiplib.set_variant(name)
    try:
        yield
    finally:
        hiplib.set_variant("auto")


# ---- multiexp_lane through the C ABI against the oracle's MODEL_EXP ----------------------------------------------
def exp_pair(V, T, num_exps, dt, seed, f64=False, **opts):
    """the same problem twice: for the oracle (and the built-in lane kernel) as the exponential model, for the
    library's kernels as its body (same parameters, priors and initial posterior image)"""
    ref, y = cases.exp_problem(V, T, num_exps, dt, seed=seed, **opts)
    if f64:
        y = y.astype(np.float64) + 1e-9  # (not representable in float32)
    mvn = hiplib.initial_mvn(ref, y)
    ref, _ = cases.exp_problem(V, T, num_exps, dt, seed=seed, init_mvn=mvn, **opts)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_lane", num_exps=num_exps, dt=dt, init_mvn=mvn,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **opts)
    return ref, dev, y


# (options, float64 series, the kernel of FVB_LANE_CASE this takes)
EXP_CASES = {
    "white": (dict(), False, "lane<multiexp_lane,2>"),  # float tiles
    "F counted": (dict(need_f=True), False, "lane<multiexp_lane,2,F>"),  # float tiles, detector counts iterations
    "F watched": (dict(need_f=True, convergence="trialmode"), False, "lane<multiexp_lane,2,F>"),  # ... watches F: save buffer
    "float64": (dict(need_f=True, convergence="trialmode"), True, "lane<multiexp_lane,2,F>"),  # double tiles
    "float64 counted": (dict(need_f=True), True, "lane<multiexp_lane,2,F>"),
    "masked timepoint": (dict(masked_timepoints=(5,)), False, "lane<multiexp_lane,2>"),  # in-place feed
    "masked timepoint,F": (dict(masked_timepoints=(5,), need_f=True), False, "lane<multiexp_lane,2,F>"),
}


@pytest.mark.parametrize("case", sorted(EXP_CASES))
def test_multiexp_lane_against_the_oracle(library, case):
    """The body computes the expression of the built-in exponential model, pointwise as the oracle does: held to the
    conditions tests/test_device_model.py holds wave<multiexp_dev> to (parity.strict at its base tolerances, no raised
    floor; means within 1e-6; status and iteration counts equal)."""
    opts, f64, kernel = EXP_CASES[case]
    ref, dev, y = exp_pair(197, 21, 1, 0.04, seed=20260102, f64=f64, max_iterations=10, **opts)
    with variant("lane"):
        assert hiplib.kernel_name(dev) == kernel
        got = hiplib.run_host(dev, y)
    r = parity.strict(ref, oracle.run(ref, y), got, what="multiexp_lane " + case, cpu2=oracle.run_fma(ref, y))
    print("multiexp_lane %s: err means %.3e cov %.3e F %.3e" % (case, r["err_means"], r["err_cov"], r["err_f"]))
    assert not r["raised"]
    assert r["err_means"] < 1e-6


def test_biexponential_needs_no_bound_the_builtin_kernel_does_not_need(library):
    """P = 4, two iterations (the bi-exponential fit is chaotic over many): lane<multiexp_lane,4> and the
    built-in lane<exp,4> on the same problem against the oracle"""
    ref, dev, y = exp_pair(197, 21, 2, 0.04, seed=20260103, max_iterations=2, need_f=True)
    cpu, cpu2 = oracle.run(ref, y), oracle.run_fma(ref, y)
    with variant("lane"):
        assert hiplib.kernel_name(dev) == "lane<multiexp_lane,4,F>" and hiplib.kernel_name(ref) == "lane<exp,4,F>"
        lib, builtin = hiplib.run_host(dev, y), hiplib.run_host(ref, y)
    r_builtin = parity.strict(ref, cpu, builtin, what="lane<exp,4,F>", cpu2=cpu2, allow_floor=True)
    print("lane<exp,4,F>: err means %.3e cov %.3e F %.3e raised %s" % (r_builtin["err_means"], r_builtin["err_cov"], r_builtin["err_f"], r_builtin["raised"]))
    r_lib = parity.strict(ref, cpu, lib, what="lane<multiexp_lane,4,F>", cpu2=cpu2, allow_floor=True)
    print("lane<multiexp_lane,4,F>: err means %.3e cov %.3e F %.3e raised %s" % (r_lib["err_means"], r_lib["err_cov"], r_lib["err_f"], r_lib["raised"]))
    assert r_builtin["raised"] or not r_lib["raised"]


# ---- invrec_lane ---------------------------------------------------------------------------------------------------
TIS = np.linspace(0.1, 4.0, 16)
INVREC_PARAMS = [dict(name="M0", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
                 dict(name="T1", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG),
                 dict(name="a", prior=(0.8, 4.0), post=(0.8, 1.0), prior_type="N", transform=vbabi.TRANSFORM_FRACTIONAL)]


def invrec_series(V, seed, noise_sd=2.0, noise_free=()):
    """a signal of order 100 with noise of 2: F of order -40, away from zero (assert_routes_agree)"""
    rng = np.random.default_rng(seed)
    truth = dict(M0=rng.uniform(80, 120, V), T1=rng.uniform(0.8, 1.6, V), a=rng.uniform(0.85, 0.98, V))
    clean = truth["M0"] * (1 - 2 * truth["a"] * np.exp(-TIS[:, None] / truth["T1"]))
    y = clean + rng.normal(0, noise_sd, clean.shape)
    for v in noise_free:
        y[:, v] = clean[:, v]
    return y.astype(np.float32), truth


def invrec_problem(y, constants=TIS, **opts):
    """through the C ABI: the initial posterior as the library's InitVoxelPosterior sets it (M0 = max |y|)"""
    V = y.shape[1]
    h = vbabi.build_config(vbabi.MODEL_PLUGIN, V, len(TIS), device_model="invrec_lane", constants=constants, params=INVREC_PARAMS, **opts)
    mvn = hiplib.initial_mvn(h, y)
    n = 4
    mvn[n * (n + 1) // 2 + 0] = np.abs(y.astype(np.float64)).max(axis=0)
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, len(TIS), device_model="invrec_lane", constants=constants, params=INVREC_PARAMS,
                              init_mvn=mvn, **opts)


def lane_and_wave(h, y):
    with variant("lane"):
        assert hiplib.kernel_name(h).startswith("lane<invrec_lane,3")
        lane = hiplib.run_host(h, y)
    with variant("wave"):
        assert hiplib.kernel_name(h) == "wave<invrec_lane>"
        wave = hiplib.run_host(h, y)
    return lane, wave


def model_space_means(h, r):
    n = h.cfg.n_params + 1
    rows = r["mvn"][n * (n + 1) // 2:n * (n + 1) // 2 + h.cfg.n_params]
    return np.array([[vbabi.to_model(h.cfg.transform[i], float(x)) for x in rows[i]] for i in range(h.cfg.n_params)])


def assert_results_agree(h, a, b, sel=None):
    """assert_routes_agree of tests/test_device_model.py - its tolerances are a cap here - on the results of the C ABI:
    model-space means, the posterior image, F compared relatively where it stays away from zero"""
    sel = np.ones(h.cfg.n_voxels, dtype=bool) if sel is None else sel
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["iterations"], b["iterations"])
    assert np.abs(b["free_energy"][sel]).min() > 1.0, "F passes near zero: the relative comparison of F is ill-posed on this data"
    ma, mb = model_space_means(h, a)[:, sel], model_space_means(h, b)[:, sel]
    d_mean = np.max(np.abs(ma - mb) / (1e-5 + 2e-5 * np.abs(mb)))
    d_mvn = np.max(np.abs(a["mvn"][:, sel] - b["mvn"][:, sel]) / (1e-7 + 1e-4 * np.abs(b["mvn"][:, sel])))
    d_f = np.max(np.abs(a["free_energy"][sel] - b["free_energy"][sel]) / (1e-8 + 1e-5 * np.abs(b["free_energy"][sel])))
    print("lane against wave, as fractions of the tolerances (means rtol 2e-5 atol 1e-5, MVN rtol 1e-4 atol 1e-7, F rtol 1e-5): "
          "means %.3e MVN %.3e F %.3e; max |d mean| %.3e, max relative dF %.3e"
          % (d_mean, d_mvn, d_f, np.max(np.abs(ma - mb)), np.max(np.abs(a["free_energy"][sel] - b["free_energy"][sel]) / np.abs(b["free_energy"][sel]))))
    assert d_mean <= 1 and d_mvn <= 1 and d_f <= 1


def test_invrec_lane_route_against_the_wave_route_of_the_same_body(library):
    """... with four noise-free voxels: the moment form of k'k cancels there and the rescue evaluates the
    body from the parameters parked in LDS, reading the constants"""
    noise_free = (3, 64, 130, 196)
    y, _ = invrec_series(197, seed=51, noise_free=noise_free)
    h = invrec_problem(y, need_f=True, max_iterations=6)
    lane, wave = lane_and_wave(h, y)
    assert np.all(wave["status"] == 0)
    assert_results_agree(h, lane, wave)
    ml, mw = model_space_means(h, lane)[:, list(noise_free)], model_space_means(h, wave)[:, list(noise_free)]
    print("noise-free voxels: max |d mean| %.3e, noise precision lane %s wave %s"
          % (np.max(np.abs(ml - mw)), lane["mvn"][13, list(noise_free)], wave["mvn"][13, list(noise_free)]))


def test_last_partial_wavefront(library):
    """voxel 64 of a run of 65 voxels (alone in its wavefront, 63 lanes repeating it) is bit for bit the voxel 64 of a
    run of 128"""
    y, _ = invrec_series(128, seed=52)
    big = invrec_problem(y, need_f=True, max_iterations=6)
    y65 = np.ascontiguousarray(y[:, :65])
    small = invrec_problem(y65, need_f=True, max_iterations=6)
    with variant("lane"):
        a, b = hiplib.run_host(small, y65), hiplib.run_host(big, y)
    assert np.all(b["status"] == 0)
    for k in ("mvn", "free_energy", "status", "iterations"):
        assert np.array_equal(a[k][..., 64], b[k][..., 64]), k
        assert np.array_equal(a[k][..., :64], b[k][..., :64]), k


def invrec_options(**extra):
    opts = {"model": "invrec_lane", "noise": "white", "method": "vb", "max-iterations": 6, "save-mean": True, "save-mvn": True,
            "save-free-energy": True, "save-model-fit": True, "save-residuals": True}
    for i, ti in enumerate(TIS):
        opts["ti%d" % (i + 1)] = float(ti)
    opts.update(extra)
    return opts


def test_through_fabber_run_against_the_host_model_route(library):
    """a 16 x 16 x 16 volume: 4096 voxels take the lane kernels without being asked to"""
    from test_device_model import assert_routes_agree
    y, _ = invrec_series(4096, seed=53)
    data = y.T.reshape(16, 16, 16, len(TIS)).copy()
    opts = invrec_options()
    dev = fabber.run(data, opts, model_libs=[library])
    host = fabber.run(data, dict(opts, **{"host-model": True}), model_libs=[library])
    assert "with the body 'invrec_lane' of its library" in dev["log"]
    assert "kernel lane<invrec_lane,3,F>, 4096 voxels x 16 timepoints" in dev["log"]  # (F is saved: the kernels with F)
    assert "evaluated on the host" in host["log"] and "of its library" not in host["log"]
    assert_routes_agree(dev, host, ("mean_M0", "mean_T1", "mean_a"))
    assert np.allclose(dev["modelfit"] + dev["residuals"], data, rtol=0, atol=1e-4)
    # without F the run takes the kernels without it
    plain = fabber.run(data, {k: v for k, v in opts.items() if k != "save-free-energy"}, model_libs=[library])
    assert "kernel lane<invrec_lane,3>, 4096 voxels" in plain["log"]


def test_blocks_of_the_host_entry_point_are_the_run_in_one(library, monkeypatch):
    """every block takes the lane kernel (the choice is made for the whole problem's voxel count) and gets the
    constants; the last block ends in a partial wavefront"""
    y, _ = invrec_series(4096 + 37, seed=54)
    h = invrec_problem(y, need_f=True, max_iterations=6)
    assert hiplib.kernel_name(h) == "lane<invrec_lane,3,F>"
    monkeypatch.setenv("FVB_HOST_BLOCK_VOXELS", "0")
    one = hiplib.run_host(h, y)
    monkeypatch.setenv("FVB_HOST_BLOCK_VOXELS", "1024")
    many = hiplib.run_host(h, y)
    for k in ("mvn", "free_energy", "status", "iterations"):
        assert np.array_equal(one[k], many[k]), k
    assert np.all(one["status"] == 0)


def test_a_failing_voxel_has_the_status_of_the_wave_route(library):
    """a non-finite sample: that voxel alone carries the status the wave route gives it"""
    y, _ = invrec_series(197, seed=55)
    y[5, 70] = np.nan
    h = invrec_problem(y, need_f=True, max_iterations=6)
    # (M0 starts at max |y|: of the finite samples, as neither route may start from NaN to get this far)
    n = 4
    h.keep["init_mvn"][n * (n + 1) // 2, 70] = np.nanmax(np.abs(y[:, 70]))
    lane, wave = lane_and_wave(h, y)
    assert wave["status"][70] != 0 and lane["status"][70] == wave["status"][70]
    assert lane["setup_failed"][70] == wave["setup_failed"][70]
    rest = np.ones(197, dtype=bool)
    rest[70] = False
    assert np.all(lane["status"][rest] == 0)
    assert_results_agree(h, lane, wave, rest)


def test_too_few_constants_stop_every_voxel_in_its_set_up(library):
    """15 inversion times for 16 timepoints: the body answers the timepoint without a constant with a non-finite
    prediction - nothing is read past the constants block - and every voxel stops on the non-finite offset"""
    y, _ = invrec_series(197, seed=56)
    h = invrec_problem(y)
    short = vbabi.build_config(vbabi.MODEL_PLUGIN, 197, len(TIS), device_model="invrec_lane", constants=TIS[:-1], params=INVREC_PARAMS,
                               init_mvn=h.keep["init_mvn"])
    with variant("lane"):
        assert hiplib.kernel_name(short) == "lane<invrec_lane,3>"
        r = hiplib.run_host(short, y)
    assert np.all(r["status"] == vbabi.STATUS_BAD_OFFSET) and np.all(r["setup_failed"])


def test_device_pointers_run_the_lane_kernel(library):
    """DeviceProblem names the lane kernel and uploads the constants block; the device entry point against the host
    entry point, bit for bit"""
    from fabber_core_amd.device import DeviceProblem
    y, _ = invrec_series(4096, seed=57)
    h = invrec_problem(y, max_iterations=6)
    host = hiplib.run_host(h, y)
    prob = DeviceProblem(h, y, "cuda:0")
    assert prob.kernel == "lane<invrec_lane,3>"
    prob.run()
    dev = prob.results()
    assert np.array_equal(host["mvn"], dev["mvn"]) and np.array_equal(host["status"], dev["status"])
    assert np.all(host["status"] == 0)
