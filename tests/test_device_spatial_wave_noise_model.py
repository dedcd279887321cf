"""Spatial VB around the device body of a model library with ONE WAVEFRONT per voxel under a NOISE PATTERN
(include/fabber_device_spatial_wave_noise_model.h): the set-up kernel and the second sweep of the wave-per-voxel spatial
family in their form for 2 to 8 noise precisions, compiled in the library's code object around the library's evaluator, and
the engine's first sweep and result image for N classes - any parameter count up to 32. Against the CPU oracle, which runs
the built-in model under the same pattern; against the lane kernels where a count has them; through fabber_dorun
(tests/plugins/fwdmodel_spatial_wave_noise_models.hip: multiexp_spwn, linear_spwn, suppconv_spwn, multiexp_spwn_both).

The volume is that of tests/test_device_spatial_wave_model.py: 7 x 6 x 5 masked to about 174 voxels, every voxel a
workgroup. The shapes are the smallest at which these kernels can go wrong: T = 21 is one partial chunk of the 64
timepoints staged at a time, T = 70 a full chunk and a partial one with the classes running across the boundary at t = 64;
pattern 12312 gives unequal class counts; P = 32 with 8 precisions is the largest layout (89.8 KB of LDS); P = 2 with 5
precisions is a count with lane kernels for 2 to 4 precisions only. The yardsticks are the project's own: parity.strict with
the oracle's FMA build as cpu2, allow_floor=True only for the exponential model (as tests/test_spatial_wide.py), status and
iteration counts the oracle's; no raised bound is accepted."""
import numpy as np
import pytest

import device_model_lib
import device_spatial_wave_noise_lib
import oracle
import parity
from fabber_core_amd import fabber, hiplib, vbabi
from test_device_spatial_model import SHAPE
from test_device_spatial_wave_model import oracle_pair
from test_spatial import masked_volume
from test_spatial_wide import MIXED, cosine_design, smooth_linear_data

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]

NAMES = device_spatial_wave_noise_lib.NAMES


@pytest.fixture(scope="module")
def library():
    assert hiplib.available() and hiplib.device_count() > 0
    path = device_spatial_wave_noise_lib.build_spatial_wave_noise_library()
    hiplib.load_model_library(path)
    assert set(NAMES) <= set(hiplib.device_models()) and set(NAMES) <= set(hiplib.device_spatial_wave_noise_models())
    assert not set(NAMES) & set(hiplib.device_spatial_wave_models())  # (the noise line does not need the white line)
    return path


@pytest.fixture(scope="module")
def volume():
    mask, coords = masked_volume(SHAPE, seed=61, keep=0.85)
    V = coords.shape[1]
    assert 128 < V < 192 and len(set(coords[2].tolist())) == 5
    return mask, coords


def wave_name(name, pattern):
    return "spatial<%s,wave,phis%d>" % (name, len(set(pattern)))


def against_the_oracle(ref, dev, coords, y, name, what, exp1ulp=False, **kw):
    """parity.strict of the library's run against the oracle's run of the built-in model; status and iteration counts the
    oracle's (parity.strict asserts them), nothing raised"""
    assert hiplib.spatial_kernel_name(dev) == name
    sp = vbabi.SpatialHolder(coords)
    cpu, cpu2 = oracle_pair(ref, sp, y, exp1ulp=exp1ulp)
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


# ---- 1. linear_spwn against the oracle's MODEL_LINEAR under the same pattern ----------------------------------------------
def linear_problem(coords, P, T, pattern, need_f, masked=(), iters=5, init_mvn=None):
    """(ref, dev, y): the design of P cosine regressors with the mixed priors of tests/test_spatial_wide.py (M, M, m, P, p,
    ARD, an image prior, then N; the first P of them) for the oracle as the built-in linear model and for the library as
    linear_spwn with the design in its constants block, both under noise-pattern `pattern`; the same initial posterior image
    with one noise row per class and the means 1 / (k + 1) (away from zero: the reference's difference step is then 1e-5 of
    the mean and not its floor of 1e-10)"""
    V = coords.shape[1]
    X = cosine_design(T, P)
    _, y = smooth_linear_data(coords, X, seed=P + 1)
    ov = {"Parameter_%d" % (k + 1): dict(type=t) for k, t in enumerate(MIXED[:P])}
    images = {}
    k_img = MIXED.index("I")
    if k_img < P:
        ov["Parameter_%d" % (k_img + 1)] = dict(type="I", prec=4.0)
        images["Parameter_%d" % (k_img + 1)] = 0.2 + 0.05 * np.cos(coords[0] / 2.0)
    common = dict(max_iterations=iters, need_f=need_f, param_overrides=ov, masked_timepoints=masked, image_priors=images,
                  noise_pattern=pattern)
    mvn = init_mvn
    if mvn is None:
        mvn = hiplib.initial_mvn(vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, **common), y)
        n = P + len(set(pattern))
        assert mvn.shape[0] == vbabi.mvn_rows(n)
        for k in range(P):
            mvn[n * (n + 1) // 2 + k] = 1.0 / (k + 1)
    ref = vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, init_mvn=mvn, **common)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="linear_spwn", constants=X,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_LINEAR, n_basis=P), init_mvn=mvn, **common)
    assert dev.cfg.n_phis == len(set(pattern)) == ref.cfg.n_phis
    return ref, dev, y


LINEAR_CASES = [(7, 21, "12", ()), (7, 21, "123", (4, 17)), (10, 70, "12312", ()), (32, 70, "12345678", ()), (2, 21, "12345", ())]


@pytest.mark.parametrize("P,T,pattern,masked", LINEAR_CASES)
@pytest.mark.parametrize("need_f", [False, True])
def test_linear_spwn_against_the_oracle(library, volume, P, T, pattern, masked, need_f):
    _, coords = volume
    ref, dev, y = linear_problem(coords, P, T, pattern, need_f, masked=masked)
    assert np.count_nonzero(dev.keep["phi_index"] == 255) == len(masked)
    cpu, got = against_the_oracle(ref, dev, coords, y, wave_name("linear_spwn", pattern),
                                  "P=%d T=%d pattern %s need_f=%d" % (P, T, pattern, need_f), check_f=need_f)
    assert np.all(got["status"] == 0) and np.isfinite(got["mvn"]).all()
    if need_f:
        assert np.isfinite(got["free_energy"]).all()


# ---- 2. multiexp_spwn against the oracle's MODEL_EXP ----------------------------------------------------------------------
def exp_problem(coords, num, device_model="multiexp_spwn", pattern="12", T=60, **opts):
    """the construction of exp_problem in tests/test_device_spatial_wave_model.py (well-separated rates in the initial image,
    a prior M on amp1) under a noise pattern, with one noise row per class in the image"""
    V, dt = coords.shape[1], 0.01
    rates, amps = np.array([0.5, 3.0, 12.0, 40.0, 150.0])[:num], np.array([1.0, 0.8, 0.6, 0.4, 0.3])[:num]
    rng = np.random.default_rng(22)
    t = np.arange(T) * dt
    scale = 1.0 + 0.2 * np.sin(coords[0] / 2.0)
    y = sum(amps[i] * scale[None, :] * np.exp(-rates[i] * t)[:, None] for i in range(num)) + rng.normal(0, 0.02, (T, V))
    init = hiplib.initial_mvn(vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=num, dt=dt, noise_pattern=pattern), y)
    n = 2 * num + len(set(pattern))
    nCov = n * (n + 1) // 2
    assert init.shape[0] == vbabi.mvn_rows(n)
    for i in range(num):
        init[nCov + 2 * i] = np.log(amps[i])
        init[nCov + 2 * i + 1] = np.log(rates[i])
    common = dict(num_exps=num, dt=dt, init_mvn=init, param_overrides={"amp1": dict(type="M")}, noise_pattern=pattern, **opts)
    ref = vbabi.build_config(vbabi.MODEL_EXP, V, T, **common)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=device_model,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num), **common)
    return ref, dev, y


def test_multiexp_spwn_against_the_oracle(library, volume):
    """five exponentials (P = 10) over three iterations under pattern 12"""
    _, coords = volume
    ref, dev, y = exp_problem(coords, 5, max_iterations=3)
    cpu, got = against_the_oracle(ref, dev, coords, y, "spatial<multiexp_spwn,wave,phis2>", "5 exponentials", exp1ulp=True, allow_floor=True)
    assert np.isfinite(got["mvn"][:, got["status"] == 0]).all()


# ---- 3. failing voxels ----------------------------------------------------------------------------------------------------
def test_voxels_that_fail_are_ignored_by_their_neighbours_as_in_the_oracle(library, volume):
    """a NaN and an Inf sample in two voxels under pattern 12, P = 7: statuses and every other voxel as the oracle has them"""
    _, coords = volume
    ref, dev, y = linear_problem(coords, 7, 21, "12", True)
    V = y.shape[1]
    bad = [V // 3, (2 * V) // 3]
    y[5, bad[0]] = np.nan
    y[17, bad[1]] = np.inf
    cpu, got = against_the_oracle(ref, dev, coords, y, "spatial<linear_spwn,wave,phis2>", "failed voxels", check_f=True)
    assert np.all(got["status"][bad] != 0) and np.count_nonzero(got["status"]) == len(bad)
    ok = got["status"] == 0
    assert np.isfinite(got["mvn"][:, ok]).all() and np.isfinite(got["free_energy"][ok]).all()


# ---- 4. the wave kernels against the lane kernels -------------------------------------------------------------------------
def test_wave_against_lane_at_four_parameters(library, volume):
    """multiexp_spwn_both has a lane noise line for P = 4: pattern 12 takes spatial<multiexp_spwn_both,4,pattern2> there; the
    same body under the name multiexp_spwn takes the wave kernels. Both against the oracle; different kernels, different bits"""
    _, coords = volume
    assert ("multiexp_spwn_both", 4) in hiplib.device_spatial_noise_models()
    ref, lane_cfg, y = exp_problem(coords, 2, device_model="multiexp_spwn_both", max_iterations=3)
    _, wave_cfg, _ = exp_problem(coords, 2, device_model="multiexp_spwn", max_iterations=3)
    _, lane = against_the_oracle(ref, lane_cfg, coords, y, "spatial<multiexp_spwn_both,4,pattern2>", "2 exponentials", exp1ulp=True, allow_floor=True)
    _, wave = against_the_oracle(ref, wave_cfg, coords, y, "spatial<multiexp_spwn,wave,phis2>", "2 exponentials", exp1ulp=True, allow_floor=True)
    assert not np.array_equal(lane["mvn"], wave["mvn"])
    # every other count of the name with the lane line takes the wave kernels, and so do 5 to 8 precisions at its count
    _, other, _ = exp_problem(coords, 3, device_model="multiexp_spwn_both", max_iterations=1)
    assert hiplib.spatial_kernel_name(other) == "spatial<multiexp_spwn_both,wave,phis2>"
    _, five, _ = exp_problem(coords, 2, device_model="multiexp_spwn_both", pattern="12345", max_iterations=1)
    assert hiplib.spatial_kernel_name(five) == "spatial<multiexp_spwn_both,wave,phis5>"


# ---- 5. supplementary data ------------------------------------------------------------------------------------------------
def test_suppconv_spwn_against_the_lane_spatial_route_of_suppconv_sp(library, volume):
    """the same body under two names: suppconv_sp has a lane spatial noise line for P = 2 (tests/plugins/
    fwdmodel_spatial_noise_models.hip), suppconv_spwn the wave noise line only - every voxel with its own input curve, under
    pattern 12; the comparison and the bounds of the test of this name in tests/test_device_spatial_wave_model.py"""
    from test_device_spatial_noise_model import T as T_SUPP, supp_series
    hiplib.load_model_library(device_model_lib.build("fwdmodel_spatial_noise_models.hip", (1, 2, 3, 4, 5), "libfabber_models_spatial_noise.so"))
    _, coords = volume
    supp, y = supp_series(coords, seed=72)
    V = y.shape[1]
    params = [dict(name="amp", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
              dict(name="r", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG)]

    def config(name, supp=supp, **kw):
        return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T_SUPP, device_model=name, dt=0.25, params=params, suppdata=supp,
                                  param_overrides={"amp": dict(type="M")}, max_iterations=5, need_f=True, noise_pattern="12", **kw)
    mvn = hiplib.init_posterior_host(config("suppconv_sp"), y)
    lane_cfg, wave_cfg = config("suppconv_sp", init_mvn=mvn), config("suppconv_spwn", init_mvn=mvn)
    assert hiplib.spatial_kernel_name(lane_cfg) == "spatial<suppconv_sp,2,pattern2>"
    assert hiplib.spatial_kernel_name(wave_cfg) == "spatial<suppconv_spwn,wave,phis2>"
    sp = vbabi.SpatialHolder(coords)
    lane, wave = hiplib.run_spatial_host(lane_cfg, sp, y), hiplib.run_spatial_host(wave_cfg, sp, y)
    assert np.all(lane["status"] == 0) and np.array_equal(lane["status"], wave["status"])
    lane.setdefault("f_history_len", np.zeros(V, dtype=np.int32))
    r = parity.strict(lane_cfg, lane, wave, what="spatial<suppconv_spwn,wave,phis2> against spatial<suppconv_sp,2,pattern2>", check_f=True)
    print("suppconv_spwn against suppconv_sp: err means %.3e cov %.3e F %.3e" % (r["err_means"], r["err_cov"], r["err_f"]))
    # the curves handed to the wrong voxels are far outside these bounds
    moved = hiplib.run_spatial_host(config("suppconv_spwn", supp=np.roll(supp, 1, axis=1), init_mvn=mvn), sp, y)
    n = 4
    assert np.abs(moved["mvn"][n * (n + 1) // 2] - wave["mvn"][n * (n + 1) // 2]).max() > 1e-2 * np.abs(wave["mvn"][n * (n + 1) // 2]).max()


# ---- 6. continue-from-mvn -------------------------------------------------------------------------------------------------
def test_a_run_started_from_the_first_runs_image_does_what_the_oracle_does_from_that_image(library, volume):
    """the noise posterior of every class comes back out of the rows P + k of the image (WhiteParams::InputFromMVN)"""
    _, coords = volume
    ref, dev, y = linear_problem(coords, 7, 21, "123", True, iters=3)
    first = hiplib.run_spatial_host(dev, vbabi.SpatialHolder(coords), y)
    assert np.all(first["status"] == 0)
    ref2, dev2, _ = linear_problem(coords, 7, 21, "123", True, iters=3, init_mvn=first["mvn"])
    cpu, got = against_the_oracle(ref2, dev2, coords, y, "spatial<linear_spwn,wave,phis3>", "continued", check_f=True)
    assert np.all(got["status"] == 0) and not np.array_equal(got["mvn"], first["mvn"])


# ---- 7. through fabber_dorun ----------------------------------------------------------------------------------------------
def test_multiexp_spwn_through_fabber_run(library):
    """model=multiexp_spwn num-exps=5 noise-pattern=12 method=spatialvb: with every prior N the spatial loop is the voxelwise
    one (bounds of test_model_library_with_ten_parameters_under_spatial_vb in tests/test_spatial_wide.py); with M+ it is
    not. Before these kernels the call was refused: "white noise with one noise precision"."""
    rng = np.random.default_rng(51)
    shape, T, dt = (6, 5, 4), 50, 0.01
    t = np.arange(T) * dt
    amp = 1.0 + 0.3 * (np.arange(shape[0])[:, None, None] > 2) + np.zeros(shape)
    series = sum(a * np.exp(-r * t) for a, r in zip([1.0, 0.8, 0.6, 0.4, 0.3], [0.5, 3.0, 12.0, 40.0, 150.0]))
    data = (amp[..., None] * series + rng.normal(0, 0.02, shape + (T,))).astype(np.float32)
    opts = {"model": "multiexp_spwn", "num-exps": 5, "dt": dt, "noise": "white", "noise-pattern": "12", "method": "spatialvb",
            "max-iterations": 2, "save-mean": True, "save-mvn": True, "save-noise-mean": True, "save-noise-std": True}
    plain = fabber.run(data, opts, model_libs=[library])
    assert "kernels spatial<multiexp_spwn,wave,phis2>" in plain["log"] and "the model is evaluated on the host" not in plain["log"]
    voxelwise = fabber.run(data, dict(opts, method="vb", convergence="maxits"), model_libs=[library])
    names = ["%s%d" % (nm, i + 1) for i in range(5) for nm in ("amp", "r")]
    for k in names:
        print("%s: max difference %.3e" % (k, np.abs(plain["mean_" + k] - voxelwise["mean_" + k]).max()))
        assert np.allclose(plain["mean_" + k], voxelwise["mean_" + k], rtol=2e-5, atol=1e-5), k
    assert np.allclose(plain["finalMVN"], voxelwise["finalMVN"], rtol=1e-4, atol=1e-7)
    # one noise image per class, the posterior means of the result image's noise rows
    assert plain["noise_means"].shape == shape + (2,) and plain["noise_stdevs"].shape == shape + (2,)
    n = 12
    assert np.allclose(plain["noise_means"], plain["finalMVN"][..., n * (n + 1) // 2 + 10:n * (n + 1) // 2 + 12], rtol=1e-6)
    assert np.all(plain["noise_means"] > 0) and np.abs(plain["noise_means"][..., 0] - plain["noise_means"][..., 1]).max() > 0
    smooth = fabber.run(data, dict(opts, **{"param-spatial-priors": "M+"}), model_libs=[library])
    assert "kernels spatial<multiexp_spwn,wave,phis2>" in smooth["log"]
    assert all(np.isfinite(smooth["mean_" + k]).all() for k in names) and np.isfinite(smooth["finalMVN"]).all()
    assert max(np.abs(smooth["mean_" + k] - voxelwise["mean_" + k]).max() for k in names) > 1e-3  # (the spatial prior did something)
