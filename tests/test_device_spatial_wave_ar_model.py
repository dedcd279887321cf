"""Spatial VB around the device body of a model library with ONE WAVEFRONT per voxel under AR(1) NOISE
(include/fabber_device_spatial_wave_ar_model.h): the set-up kernel and the second sweep of the wave-per-voxel spatial family
in their AR(1) form (one echo, no cross terms), compiled in the library's code object around the library's evaluator, and
the engine's first sweep and result image for it - any parameter count up to 32. Against the CPU oracle, which runs the
built-in model under noise=ar; against the lane kernels where a count has them; through fabber_dorun
(tests/plugins/fwdmodel_spatial_wave_ar_models.hip: multiexp_spwa, linear_spwa, suppconv_spwa, multiexp_spwa_both).

The volume is that of tests/test_device_spatial_wave_model.py: 7 x 6 x 5 masked to about 174 voxels, every voxel a
workgroup. The lag-1 moments are summed over chunks of 64 timepoints with the last row of a chunk carried into the next: the
(P, T) of device_spatial_wave_ar_lib.LINEAR_CASES are the shapes at which that can go wrong. The yardsticks are the
project's own: parity.strict with the oracle's FMA build as cpu2, allow_floor=True only for the exponential model, status
and iteration counts the oracle's; no raised bound is accepted.

The tests without the gpu mark hold the ORACLE to what the GPU tests ask: on every problem no voxel fails but the planted
ones, the two CPU builds take the same number of iterations and lie within a third of the base tolerances of each other -
the GPU cases are ones the reference's own arithmetic holds without a raised bound. (The seeds are the sibling tests';
none had to be changed for that.)"""
import numpy as np
import pytest

import device_model_lib
import device_spatial_wave_ar_lib as arlib
import oracle
import parity
from fabber_core_amd import fabber, hiplib, vbabi
from test_device_spatial_wave_model import oracle_pair

pytestmark = [pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]
gpu = pytest.mark.gpu

NAMES = arlib.NAMES


@pytest.fixture(scope="module")
def library():
    assert hiplib.available() and hiplib.device_count() > 0
    path = arlib.build_spatial_wave_ar_library()
    hiplib.load_model_library(path)
    assert set(NAMES) <= set(hiplib.device_models()) and set(NAMES) <= set(hiplib.device_spatial_wave_ar_models())
    # (the AR line needs neither the white line nor the pattern line)
    assert not set(NAMES) & set(hiplib.device_spatial_wave_models()) and not set(NAMES) & set(hiplib.device_spatial_wave_noise_models())
    return path


@pytest.fixture(scope="module")
def volume():
    return arlib.volume()


@pytest.fixture(scope="module")
def cases(volume):
    return arlib.oracle_cases(volume[1])


@pytest.fixture(scope="module")
def oracle_runs(volume, cases):
    """the oracle's runs of every case, computed once: name -> (cpu, [cpu2 ...])"""
    sp = vbabi.SpatialHolder(volume[1])
    return {name: oracle_pair(ref, sp, y, exp1ulp=exp1ulp) for name, (ref, dev, y, exp1ulp, bad) in cases.items()}


def wave_name(name):
    return "spatial<%s,wave,ar1>" % name


def against_the_oracle(ref, dev, coords, y, name, what, exp1ulp=False, runs=None, **kw):
    """parity.strict of the library's run against the oracle's run of the built-in model; status and iteration counts the
    oracle's (parity.strict asserts them), nothing raised"""
    assert hiplib.spatial_kernel_name(dev) == name
    sp = vbabi.SpatialHolder(coords)
    cpu, cpu2 = runs if runs is not None else oracle_pair(ref, sp, y, exp1ulp=exp1ulp)
    got = hiplib.run_spatial_host(dev, sp, y)
    ok = (cpu["status"] == 0) & (got["status"] == 0) & (cpu["iterations"] == got["iterations"])
    e_mean, e_cov, _ = parity.voxel_errors(ref, cpu, got, ok)  # (the figures, before anything is asserted)
    print("%s %s: err means %.3e cov %.3e, status differs on %d voxels" % (name, what, e_mean.max(), e_cov.max(),
                                                                         np.count_nonzero(cpu["status"] != got["status"])))
    r = parity.strict(ref, cpu, got, what=name + " " + what, cpu2=cpu2, **kw)
    print("%s %s: err means %.3e cov %.3e F %.3e raised %s" % (name, what, r["err_means"], r["err_cov"], r["err_f"], r["raised"]))
    assert kw.get("allow_floor") or not r["raised"]
    assert np.array_equal(got["status"], cpu["status"]) and np.array_equal(got["iterations"], cpu["iterations"])
    return cpu, got


def noise_rows(mvn, P):
    """(alpha_1, alpha_2, phi) means of a result image"""
    n = P + 3
    return mvn[n * (n + 1) // 2 + P:n * (n + 1) // 2 + n]


# ---- 1. linear_spwa against the oracle's MODEL_LINEAR under noise=ar -------------------------------------------------------
@gpu
@pytest.mark.parametrize("P,T", arlib.LINEAR_CASES)
@pytest.mark.parametrize("need_f", [False, True])
def test_linear_spwa_against_the_oracle(library, volume, cases, oracle_runs, P, T, need_f):
    _, coords = volume
    key = "linear P=%d T=%d need_f=%d" % (P, T, need_f)
    ref, dev, y, _, _ = cases[key]
    cpu, got = against_the_oracle(ref, dev, coords, y, wave_name("linear_spwa"), key, runs=oracle_runs[key], check_f=need_f)
    assert np.all(got["status"] == 0) and np.isfinite(got["mvn"]).all()
    # the three noise rows are the oracle's (alpha_2 is never updated; alpha_1 is)
    a_cpu, a_got = noise_rows(cpu["mvn"], P), noise_rows(got["mvn"], P)
    print("%s: alpha_1 in [%.3f, %.3f], largest difference %.3e" % (key, a_cpu[0].min(), a_cpu[0].max(), np.abs(a_cpu[0] - a_got[0]).max()))
    assert np.abs(a_got[0]).max() > 1e-3 and np.all(a_got[1] == 0) and np.all(a_got[2] > 0)
    if need_f:
        assert np.isfinite(got["free_energy"]).all()


# ---- 2. multiexp_spwa against the oracle's MODEL_EXP ----------------------------------------------------------------------
@gpu
def test_multiexp_spwa_against_the_oracle(library, volume, cases, oracle_runs):
    """five exponentials (P = 10) over three iterations"""
    _, coords = volume
    ref, dev, y, _, _ = cases["five exponentials"]
    cpu, got = against_the_oracle(ref, dev, coords, y, wave_name("multiexp_spwa"), "5 exponentials", runs=oracle_runs["five exponentials"],
                                  allow_floor=True)
    assert np.isfinite(got["mvn"][:, got["status"] == 0]).all()


# ---- 3. failing voxels ----------------------------------------------------------------------------------------------------
@gpu
def test_voxels_that_fail_are_ignored_by_their_neighbours_as_in_the_oracle(library, volume, cases, oracle_runs):
    """a NaN and an Inf sample in two voxels, P = 7: statuses and every other voxel as the oracle has them"""
    _, coords = volume
    ref, dev, y, _, bad = cases["failed voxels"]
    cpu, got = against_the_oracle(ref, dev, coords, y, wave_name("linear_spwa"), "failed voxels", runs=oracle_runs["failed voxels"], check_f=True)
    assert np.all(got["status"][bad] != 0) and np.count_nonzero(got["status"]) == len(bad)
    ok = got["status"] == 0
    assert np.isfinite(got["mvn"][:, ok]).all() and np.isfinite(got["free_energy"][ok]).all()


# ---- 4. continue-from-mvn -------------------------------------------------------------------------------------------------
@gpu
def test_a_run_started_from_the_first_runs_image_does_what_the_oracle_does_from_that_image(library, volume):
    """the alpha posterior and phi's come back out of the rows P, P + 1, P + 2 of the image (Ar1cParams::InputFromMVN)"""
    _, coords = volume
    ref, dev, y = arlib.linear_problem(coords, 7, 21, True, iters=3)
    first = hiplib.run_spatial_host(dev, vbabi.SpatialHolder(coords), y)
    assert np.all(first["status"] == 0) and np.abs(noise_rows(first["mvn"], 7)[0]).max() > 1e-3
    ref2, dev2, _ = arlib.linear_problem(coords, 7, 21, True, iters=3, init_mvn=first["mvn"])
    cpu, got = against_the_oracle(ref2, dev2, coords, y, wave_name("linear_spwa"), "continued", check_f=True)
    assert np.all(got["status"] == 0) and not np.array_equal(got["mvn"], first["mvn"])


# ---- 5. the alphas' prior and posterior from file -------------------------------------------------------------------------
@gpu
def test_alpha_distributions_from_file(library, volume, cases, oracle_runs):
    """an informative noise-initial-prior with an off-diagonal precision and a noise-initial-posterior with a covariance
    between the alphas (in the configuration and, as Vb::BuildInitialMvn writes it, in the initial image): the prior enters
    UpdateAlpha and three terms of F"""
    _, coords = volume
    ref, dev, y, _, _ = cases["alphas from file"]
    assert dev.cfg.ar_alpha_given == 3
    cpu, got = against_the_oracle(ref, dev, coords, y, wave_name("linear_spwa"), "alphas from file", runs=oracle_runs["alphas from file"],
                                  check_f=True)
    _, plain, _ = arlib.linear_problem(coords, 7, 21, True)
    plain = hiplib.run_spatial_host(plain, vbabi.SpatialHolder(coords), y)
    assert np.abs(got["free_energy"] - plain["free_energy"]).max() > 1e-3
    assert np.abs(noise_rows(got["mvn"], 7)[1]).max() > 1e-3  # (alpha_2's mean moves with alpha_1 through the prior's off-diagonal)


# ---- 6. the wave kernels against the lane kernels -------------------------------------------------------------------------
@gpu
def test_wave_against_lane_at_four_parameters(library, volume, cases, oracle_runs):
    """multiexp_spwa_both has a lane AR(1) line for P = 4: it takes spatial<multiexp_spwa_both,4,ar1> there; the same body under
    the name multiexp_spwa takes the wave kernels. Both against the oracle; different kernels, different bits"""
    _, coords = volume
    assert ("multiexp_spwa_both", 4) in hiplib.device_spatial_noise_models()
    ref, wave_cfg, y, _, _ = cases["two exponentials"]
    _, lane_cfg, _ = arlib.exp_problem(coords, 2, device_model="multiexp_spwa_both", max_iterations=3)
    runs = oracle_runs["two exponentials"]
    _, lane = against_the_oracle(ref, lane_cfg, coords, y, "spatial<multiexp_spwa_both,4,ar1>", "2 exponentials", runs=runs, allow_floor=True)
    _, wave = against_the_oracle(ref, wave_cfg, coords, y, wave_name("multiexp_spwa"), "2 exponentials", runs=runs, allow_floor=True)
    assert not np.array_equal(lane["mvn"], wave["mvn"])
    # every other count of the name with the lane line takes the wave kernels
    for num in (1, 3, 5):
        _, other, _ = arlib.exp_problem(coords, num, device_model="multiexp_spwa_both", max_iterations=1)
        assert hiplib.spatial_kernel_name(other) == wave_name("multiexp_spwa_both")


# ---- 7. supplementary data ------------------------------------------------------------------------------------------------
@gpu
def test_suppconv_spwa_against_the_lane_spatial_route_of_suppconv_sp(library, volume):
    """the same body under two names: suppconv_sp has a lane spatial noise line for P = 2 with the AR(1) family (tests/plugins/
    fwdmodel_spatial_noise_models.hip), suppconv_spwa the wave AR line only - every voxel with its own input curve; the
    comparison and the bounds of the test of this name in tests/test_device_spatial_wave_model.py"""
    from test_device_spatial_noise_model import T as T_SUPP, supp_series
    hiplib.load_model_library(device_model_lib.build("fwdmodel_spatial_noise_models.hip", (1, 2, 3, 4, 5), "libfabber_models_spatial_noise.so"))
    _, coords = volume
    supp, y = supp_series(coords, seed=72)
    V = y.shape[1]
    params = [dict(name="amp", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
              dict(name="r", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG)]

    def config(name, supp=supp, **kw):
        return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T_SUPP, device_model=name, dt=0.25, params=params, suppdata=supp,
                                  param_overrides={"amp": dict(type="M")}, max_iterations=5, need_f=True, **arlib.AR, **kw)
    mvn = hiplib.init_posterior_host(config("suppconv_sp"), y)
    lane_cfg, wave_cfg = config("suppconv_sp", init_mvn=mvn), config("suppconv_spwa", init_mvn=mvn)
    assert hiplib.spatial_kernel_name(lane_cfg) == "spatial<suppconv_sp,2,ar1>"
    assert hiplib.spatial_kernel_name(wave_cfg) == wave_name("suppconv_spwa")
    sp = vbabi.SpatialHolder(coords)
    lane, wave = hiplib.run_spatial_host(lane_cfg, sp, y), hiplib.run_spatial_host(wave_cfg, sp, y)
    assert np.all(lane["status"] == 0) and np.array_equal(lane["status"], wave["status"])
    lane.setdefault("f_history_len", np.zeros(V, dtype=np.int32))
    r = parity.strict(lane_cfg, lane, wave, what="spatial<suppconv_spwa,wave,ar1> against spatial<suppconv_sp,2,ar1>", check_f=True)
    print("suppconv_spwa against suppconv_sp: err means %.3e cov %.3e F %.3e" % (r["err_means"], r["err_cov"], r["err_f"]))
    # the curves handed to the wrong voxels are far outside these bounds
    moved = hiplib.run_spatial_host(config("suppconv_spwa", supp=np.roll(supp, 1, axis=1), init_mvn=mvn), sp, y)
    n = 5
    assert np.abs(moved["mvn"][n * (n + 1) // 2] - wave["mvn"][n * (n + 1) // 2]).max() > 1e-2 * np.abs(wave["mvn"][n * (n + 1) // 2]).max()


# ---- 8. through fabber_dorun ----------------------------------------------------------------------------------------------
@gpu
def test_multiexp_spwa_through_fabber_run(library):
    """model=multiexp_spwa num-exps=5 noise=ar method=spatialvb: with every prior N the spatial loop is the voxelwise one
    (bounds of test_model_library_with_ten_parameters_under_spatial_vb in tests/test_spatial_wide.py); with M+ it is not.
    Before these kernels the call fell back to the host route: "the model is evaluated on the host"."""
    rng = np.random.default_rng(51)
    shape, T, dt = (6, 5, 4), 50, 0.01
    t = np.arange(T) * dt
    amp = 1.0 + 0.3 * (np.arange(shape[0])[:, None, None] > 2) + np.zeros(shape)
    series = sum(a * np.exp(-r * t) for a, r in zip([1.0, 0.8, 0.6, 0.4, 0.3], [0.5, 3.0, 12.0, 40.0, 150.0]))
    data = (amp[..., None] * series + rng.normal(0, 0.02, shape + (T,))).astype(np.float32)
    opts = {"model": "multiexp_spwa", "num-exps": 5, "dt": dt, "noise": "ar", "method": "spatialvb",
            "max-iterations": 2, "save-mean": True, "save-mvn": True, "save-noise-mean": True, "save-noise-std": True}
    plain = fabber.run(data, opts, model_libs=[library])
    assert "kernels spatial<multiexp_spwa,wave,ar1>" in plain["log"] and "the model is evaluated on the host" not in plain["log"]
    voxelwise = fabber.run(data, dict(opts, method="vb", convergence="maxits"), model_libs=[library])
    names = ["%s%d" % (nm, i + 1) for i in range(5) for nm in ("amp", "r")]
    for k in names:
        print("%s: max difference %.3e" % (k, np.abs(plain["mean_" + k] - voxelwise["mean_" + k]).max()))
        assert np.allclose(plain["mean_" + k], voxelwise["mean_" + k], rtol=2e-5, atol=1e-5), k
    assert np.allclose(plain["finalMVN"], voxelwise["finalMVN"], rtol=1e-4, atol=1e-7)
    # the three noise images (alpha_1, alpha_2, phi) are the noise rows of the result image; noise_means / noise_stdevs hold
    # the first NumParams() = nPhis = 1 of them, alpha_1, as in the reference (Vb::SaveResults, inference_vb.cc:981-989)
    n = 13
    assert plain["finalMVN"].shape == shape + (n * (n + 1) // 2 + n + 1,)
    alpha1, alpha2, phi = (plain["finalMVN"][..., n * (n + 1) // 2 + 10 + k] for k in range(3))
    assert np.isfinite(alpha1).all() and np.abs(alpha1).max() > 1e-3 and np.all(alpha2 == 0) and np.all(phi > 0)
    assert plain["noise_means"].shape == shape == plain["noise_stdevs"].shape
    assert np.allclose(plain["noise_means"], alpha1, rtol=1e-6) and np.all(plain["noise_stdevs"] > 0)
    smooth = fabber.run(data, dict(opts, **{"param-spatial-priors": "M+"}), model_libs=[library])
    assert "kernels spatial<multiexp_spwa,wave,ar1>" in smooth["log"]
    assert all(np.isfinite(smooth["mean_" + k]).all() for k in names) and np.isfinite(smooth["finalMVN"]).all()
    assert max(np.abs(smooth["mean_" + k] - voxelwise["mean_" + k]).max() for k in names) > 1e-3  # (the spatial prior did something)


# ---- the oracle itself on these problems (no GPU) -------------------------------------------------------------------------
def builds_agree(ref, cpu, others, what, planted):
    """no failed voxel except the planted ones, equal iteration counts, and the CPU builds within a third of the base
    tolerances of each other (parity.TOL_MEAN, TOL_COV, TOL_F in the scaling of parity.voxel_errors and parity.strict)"""
    failed = np.flatnonzero(cpu["status"])
    assert sorted(failed.tolist()) == sorted(planted), (what, failed)
    ok = cpu["status"] == 0
    for other in others:
        assert np.array_equal(other["status"], cpu["status"]) and np.array_equal(other["iterations"], cpu["iterations"]), what
        e_mean, e_cov, _ = parity.voxel_errors(ref, cpu, other, ok)
        figures = [e_mean.max() / parity.TOL_MEAN, e_cov.max() / parity.TOL_COV]
        if ref.cfg.need_f:
            fa, fb = cpu["free_energy"][ok], other["free_energy"][ok]
            figures.append((np.abs(fa - fb) / np.maximum(1.0, np.abs(fa))).max() / parity.TOL_F)
        print("%s: CPU builds apart by %s of the base tolerances (means, covariances, F)" % (what, ", ".join("%.3f" % f for f in figures)))
        assert max(figures) < 1.0 / 3.0, (what, figures)


def test_the_oracle_holds_every_case_without_a_raised_bound(volume, cases, oracle_runs):
    for name, (ref, dev, y, exp1ulp, bad) in cases.items():
        cpu, others = oracle_runs[name]
        builds_agree(ref, cpu, others, name, bad)


def test_the_oracle_holds_the_continued_run(volume):
    """the continue-from-mvn case with the oracle's own first image in the place of the device's"""
    _, coords = volume
    sp = vbabi.SpatialHolder(coords)
    ref, _, y = arlib.linear_problem(coords, 7, 21, True, iters=3)
    first = oracle.run_spatial(ref, sp, y)
    assert np.all(first["status"] == 0)
    ref2, _, _ = arlib.linear_problem(coords, 7, 21, True, iters=3, init_mvn=first["mvn"])
    cpu, others = oracle_pair(ref2, sp, y)
    builds_agree(ref2, cpu, others, "continued", [])
