"""Spatial VB around the device body of a model library with ONE WAVEFRONT per voxel
(include/fabber_device_spatial_wave_model.h): the set-up kernel and the second sweep of the wave-per-voxel spatial family
compiled in the library's code object around the library's evaluator, which they linearise by the reference's central
differences - any parameter count up to 32. Against the CPU oracle, against the host route of the same family (the
linearisation computed on the host by the same differences and uploaded), and through fabber_dorun against the host-model
route of the same library (tests/plugins/fwdmodel_spatial_wave_models.hip: multiexp_spw, linear_spw, suppconv_spw,
multiexp_both).

The volume is that of tests/test_device_spatial_model.py: 7 x 6 x 5 masked to about 180 voxels, with holes, missing
neighbours and five z-planes; here every voxel is a workgroup. The shapes are the smallest at which these kernels can go
wrong: T = 21 is one partial chunk of the 64 timepoints staged at a time, T = 70 a full chunk and a partial one (60: one
partial chunk, the construction of tests/test_spatial_wide.py); P = 7 is odd and the smallest count without lane kernels
(row stride of J = P), 8 even, 10, and 32 the largest (9 moment entries per lane, 57.8 KB of LDS). The yardsticks are the
project's own: parity.strict with the oracle's FMA build as cpu2, allow_floor=True where tests/test_spatial_wide.py uses
it, status and iteration counts the oracle's."""
import ctypes as C

import numpy as np
import pytest

import device_model_lib
import device_spatial_wave_lib
import oracle
import parity
from fabber_core_amd import fabber, hiplib, vbabi
from test_device_spatial_model import SHAPE, volume_of
from test_spatial import masked_volume
from test_spatial_wide import MIXED, cosine_design, smooth_linear_data

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]

NAMES = ("multiexp_spw", "linear_spw", "suppconv_spw", "multiexp_both")


@pytest.fixture(scope="module")
def library():
    assert hiplib.available() and hiplib.device_count() > 0
    path = device_spatial_wave_lib.build_spatial_wave_library()
    hiplib.load_model_library(path)
    assert set(NAMES) <= set(hiplib.device_models()) and set(NAMES) <= set(hiplib.device_spatial_wave_models())
    return path


@pytest.fixture(scope="module")
def volume():
    mask, coords = masked_volume(SHAPE, seed=61, keep=0.85)
    V = coords.shape[1]
    assert 128 < V < 192 and len(set(coords[2].tolist())) == 5
    return mask, coords


def oracle_pair(ref, sp, y, exp1ulp=False):
    """the oracle and its other builds (FMA contraction; for the exponential model the exp of the device's accuracy class)"""
    cpu = [oracle.run_spatial(ref, sp, y), oracle.run_spatial_fma(ref, sp, y)]
    if exp1ulp:
        cpu.append(oracle.run_spatial_exp1ulp(ref, sp, y))
    for r in cpu:
        r.setdefault("f_history_len", np.zeros(ref.cfg.n_voxels, dtype=np.int32))
    return cpu[0], cpu[1:]


# ---- 1. linear_spw against the oracle's MODEL_LINEAR and against the host route of the family ---------------------------
def linear_problem(coords, P, T, need_f, masked=(), iters=5, constants=None):
    """(ref, dev, X, y): the design of P cosine regressors with the mixed priors of tests/test_spatial_wide.py (M, M, m, P,
    p, ARD, an image prior, then N) for the oracle as the built-in linear model and for the library as linear_spw with the
    design in its constants block; the same initial posterior image, whose means 1 / (k + 1) are away from zero: the
    reference's difference step is then 1e-5 of the mean and not its floor of 1e-10, at which one ulp of the prediction
    is 1e-6 of the Jacobian"""
    V = coords.shape[1]
    X = cosine_design(T, P)
    _, y = smooth_linear_data(coords, X, seed=P + 1)
    ov = {"Parameter_%d" % (k + 1): dict(type=t) for k, t in enumerate(MIXED)}
    k_img = MIXED.index("I")
    ov["Parameter_%d" % (k_img + 1)] = dict(type="I", prec=4.0)
    common = dict(max_iterations=iters, need_f=need_f, param_overrides=ov, masked_timepoints=masked,
                  image_priors={"Parameter_%d" % (k_img + 1): 0.2 + 0.05 * np.cos(coords[0] / 2.0)})
    mvn = hiplib.initial_mvn(vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, **common), y)
    n = P + 1
    for k in range(P):
        mvn[n * (n + 1) // 2 + k] = 1.0 / (k + 1)
    ref = vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, init_mvn=mvn, **common)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="linear_spw", constants=X if constants is None else constants,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_LINEAR, n_basis=P), init_mvn=mvn, **common)
    return ref, dev, X, y


def library_against_host_route_against_oracle(ref, dev, sp, y, X, what, monkeypatch, **kw):
    """parity.strict for the host route of the wave-per-voxel family (hiplib.recentre_callback of the same expression: the
    parent's behaviour for such a model) and for the library's kernels on the same problem - status and iteration counts
    the oracle's in both, and the library's need no raised bound the host route does not need"""
    T, P = X.shape
    assert hiplib.spatial_kernel_name(dev) == "spatial<linear_spw,wave>"
    cpu, cpu2 = oracle_pair(ref, sp, y)
    monkeypatch.setenv("FVB_SPATIAL_WIDE", "1")  # (up to 8 parameters the host route has lane kernels too)
    host = hiplib.run_spatial_hostmodel_host(ref, sp, y, hiplib.recentre_callback(lambda m, ids: m @ X.T, T, P))
    monkeypatch.delenv("FVB_SPATIAL_WIDE")
    lib = hiplib.run_spatial_host(dev, sp, y)
    for name, got in (("host route", host), ("library", lib)):  # (the figures, before anything is asserted)
        ok = (cpu["status"] == 0) & (got["status"] == 0) & (cpu["iterations"] == got["iterations"])
        e_mean, e_cov, _ = parity.voxel_errors(ref, cpu, got, ok)
        print("%s %s: err means %.3e cov %.3e, status differs on %d voxels" % (name, what, e_mean.max(), e_cov.max(),
                                                                             np.count_nonzero(cpu["status"] != got["status"])))
    r_host = parity.strict(ref, cpu, host, what="spatial<host,wave> " + what, cpu2=cpu2, **kw)
    r_lib = parity.strict(ref, cpu, lib, what="spatial<linear_spw,wave> " + what, cpu2=cpu2, **kw)
    print("spatial<linear_spw,wave> %s: err means %.3e cov %.3e F %.3e raised %s (host route: %.3e %.3e %.3e raised %s)"
          % (what, r_lib["err_means"], r_lib["err_cov"], r_lib["err_f"], r_lib["raised"], r_host["err_means"], r_host["err_cov"],
             r_host["err_f"], r_host["raised"]))
    assert r_host["raised"] or not r_lib["raised"]
    assert np.array_equal(lib["status"], host["status"]) and np.array_equal(lib["iterations"], host["iterations"])
    return cpu, lib


@pytest.mark.parametrize("P,T", [(7, 21), (32, 70)])
@pytest.mark.parametrize("need_f", [False, True])
def test_linear_spw_against_the_oracle_and_the_host_route(library, volume, monkeypatch, P, T, need_f):
    _, coords = volume
    ref, dev, X, y = linear_problem(coords, P, T, need_f)
    cpu, lib = library_against_host_route_against_oracle(ref, dev, vbabi.SpatialHolder(coords), y, X, "P=%d T=%d need_f=%d" % (P, T, need_f),
                                                         monkeypatch, check_f=need_f)
    assert np.all(lib["status"] == 0) and np.isfinite(lib["mvn"]).all()


def test_linear_spw_with_two_timepoints_masked(library, volume, monkeypatch):
    """phi_index 255 at two timepoints: they stage zeros and count for nothing, in the moments and in the residual"""
    _, coords = volume
    ref, dev, X, y = linear_problem(coords, 7, 21, True, masked=(4, 17))
    assert np.count_nonzero(dev.keep["phi_index"] == 255) == 2
    cpu, lib = library_against_host_route_against_oracle(ref, dev, vbabi.SpatialHolder(coords), y, X, "P=7 T=21, two masked", monkeypatch,
                                                         check_f=True)
    assert np.all(lib["status"] == 0)


# ---- 2. multiexp_spw against the oracle's MODEL_EXP ---------------------------------------------------------------------
def exp_problem(coords, num, device_model="multiexp_spw", **opts):
    """the construction of test_five_exponentials_with_central_differences_against_the_oracle (tests/test_spatial_wide.py):
    T = 60, well-separated rates in the initial image, a prior M on amp1 - ill-conditioned beyond a few iterations"""
    V, T, dt = coords.shape[1], 60, 0.01
    rates, amps = np.array([0.5, 3.0, 12.0, 40.0, 150.0])[:num], np.array([1.0, 0.8, 0.6, 0.4, 0.3])[:num]
    rng = np.random.default_rng(22)
    t = np.arange(T) * dt
    scale = 1.0 + 0.2 * np.sin(coords[0] / 2.0)
    y = sum(amps[i] * scale[None, :] * np.exp(-rates[i] * t)[:, None] for i in range(num)) + rng.normal(0, 0.02, (T, V))
    init = hiplib.initial_mvn(vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=num, dt=dt), y)
    nCov = (2 * num + 1) * (2 * num + 2) // 2
    for i in range(num):
        init[nCov + 2 * i] = np.log(amps[i])
        init[nCov + 2 * i + 1] = np.log(rates[i])
    common = dict(num_exps=num, dt=dt, init_mvn=init, param_overrides={"amp1": dict(type="M")}, **opts)
    ref = vbabi.build_config(vbabi.MODEL_EXP, V, T, **common)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=device_model,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num), **common)
    return ref, dev, y


@pytest.mark.parametrize("num", [4, 5])
def test_multiexp_spw_against_the_oracle(library, volume, num):
    """P = 8 and P = 10 over three iterations; the body computes the expression of the built-in exponential model"""
    _, coords = volume
    ref, dev, y = exp_problem(coords, num, max_iterations=3)
    assert hiplib.spatial_kernel_name(dev) == "spatial<multiexp_spw,wave>"
    sp = vbabi.SpatialHolder(coords)
    cpu, cpu2 = oracle_pair(ref, sp, y, exp1ulp=True)
    got = hiplib.run_spatial_host(dev, sp, y)
    assert np.isfinite(got["mvn"][:, got["status"] == 0]).all()
    r = parity.strict(ref, cpu, got, what="spatial<multiexp_spw,wave> %d exponentials" % num, cpu2=cpu2, allow_floor=True)
    print("spatial<multiexp_spw,wave> %d exponentials: err means %.3e cov %.3e raised %s" % (num, r["err_means"], r["err_cov"], r["raised"]))


# ---- 3. failing voxels ----------------------------------------------------------------------------------------------------
def test_voxels_that_fail_are_ignored_by_their_neighbours_as_in_the_oracle(library, volume):
    """the construction of the test of this name in tests/test_spatial_wide.py: a non-finite sample stops its voxel in the
    first sweep (F "before"); status and every other voxel's posterior as the oracle has them"""
    _, coords = volume
    ref, dev, X, y = linear_problem(coords, 7, 21, True)
    V = y.shape[1]
    bad = [V // 3, (2 * V) // 3]
    y[5, bad[0]] = np.nan
    y[17, bad[1]] = np.inf
    sp = vbabi.SpatialHolder(coords)
    cpu, cpu2 = oracle_pair(ref, sp, y)
    got = hiplib.run_spatial_host(dev, sp, y)
    assert np.all(got["status"][bad] != 0) and np.count_nonzero(got["status"]) == len(bad)
    parity.strict(ref, cpu, got, what="spatial<linear_spw,wave> failed voxels", cpu2=cpu2, check_f=True)
    ok = got["status"] == 0
    assert np.isfinite(got["mvn"][:, ok]).all() and np.isfinite(got["free_energy"][ok]).all()


def test_a_constants_block_one_row_short_stops_every_voxel_in_its_set_up(library, volume):
    """T - 1 rows of the design for T timepoints: the body answers the last timepoint with a non-finite prediction -
    nothing is read past the block - and every voxel stops in the set-up kernel with the non-finite-offset status"""
    _, coords = volume
    P, T = 7, 21
    X = cosine_design(T, P)
    _, dev, _, y = linear_problem(coords, P, T, False, iters=3, constants=X[:-1])
    assert dev.cfg.n_model_consts == (T - 1) * P and hiplib.spatial_kernel_name(dev) == "spatial<linear_spw,wave>"
    got = hiplib.run_spatial_host(dev, vbabi.SpatialHolder(coords), y)
    assert np.all(got["status"] == vbabi.STATUS_BAD_OFFSET) and np.all(got["setup_failed"])


# ---- 4. route choice ------------------------------------------------------------------------------------------------------
def multiexp_config(name, num_exps, V=180, T=21, **kw):
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=name, num_exps=num_exps, dt=0.04,
                              params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **kw)


def test_route_choice(library, volume):
    _, coords = volume
    assert hiplib.spatial_kernel_name(multiexp_config("multiexp_spw", 5)) == "spatial<multiexp_spw,wave>"
    assert hiplib.spatial_kernel_name(multiexp_config("multiexp_spw", 5, need_f=True)) == "spatial<multiexp_spw,wave>"
    # a lane entry for (name, P) comes first; every other count of the name takes the wave-per-voxel kernels
    assert ("multiexp_both", 2) in hiplib.device_spatial_models()
    assert hiplib.spatial_kernel_name(multiexp_config("multiexp_both", 1)) == "spatial<multiexp_both,2>"
    assert hiplib.spatial_kernel_name(multiexp_config("multiexp_both", 4)) == "spatial<multiexp_both,wave>"
    # the other noise models keep the host route: -40 from the engine
    _, _, y = exp_problem(coords, 5)
    for kw in (dict(noise=vbabi.NOISE_AR1, num_echoes=1), dict(noise_pattern="12")):
        _, dev, _ = exp_problem(coords, 5, max_iterations=2, **kw)
        assert hiplib.spatial_kernel_name(dev) == ""
        with pytest.raises(hiplib.HipEngineError, match="-40.*no spatial kernel"):
            hiplib.run_spatial_host(dev, vbabi.SpatialHolder(coords), y)


def test_what_unloading_the_library_does_removes_the_entry_and_the_route(library, volume):
    """A library that is unloaded unregisters its entries in the destructors of the macro lines' static objects. The test
    libraries stay resident after dlclose (their template instantiations carry unique symbols), so this calls what those
    destructors call: the entry is gone, the configuration has no kernel table and a run answers -40 - and with the entry
    back the route is back."""
    _, coords = volume
    entry = hiplib.find_device_spatial_wave_model("multiexp_spw")
    _, dev, y = exp_problem(coords, 5, max_iterations=1)
    hiplib.unregister_device_spatial_wave_model("multiexp_spw")
    try:
        assert "multiexp_spw" not in hiplib.device_spatial_wave_models() and "multiexp_both" in hiplib.device_spatial_wave_models()
        assert hiplib.find_device_spatial_wave_model("multiexp_spw") is None and hiplib.spatial_kernel_name(dev) == ""
        with pytest.raises(hiplib.HipEngineError, match="-40.*no spatial kernel"):
            hiplib.run_spatial_host(dev, vbabi.SpatialHolder(coords), y)
    finally:
        # (the registry keeps the descriptor's address until the library unregisters the name when the process ends: the
        # copy lives in memory that is never freed; its name and launcher are the library's own)
        libc = C.CDLL(None)
        libc.malloc.restype = C.c_void_p
        keep = libc.malloc(C.sizeof(entry))
        C.memmove(keep, C.byref(entry), C.sizeof(entry))
        hiplib.register_device_spatial_wave_model(C.cast(keep, C.POINTER(vbabi.FvbDeviceSpatialWaveModel)).contents)
    assert hiplib.spatial_kernel_name(dev) == "spatial<multiexp_spw,wave>"
    assert np.all(hiplib.run_spatial_host(dev, vbabi.SpatialHolder(coords), y)["status"] == 0)


# ---- 5. supplementary data ------------------------------------------------------------------------------------------------
def test_suppconv_spw_against_the_lane_spatial_route_of_suppconv_sp(library, volume):
    """the same body under two names: suppconv_sp has a lane spatial line for P = 2 (tests/plugins/
    fwdmodel_spatial_noise_models.hip), suppconv_spw the wave line only - every voxel with its own input curve"""
    from test_device_spatial_noise_model import T as T_SUPP, supp_series
    hiplib.load_model_library(device_model_lib.build("fwdmodel_spatial_noise_models.hip", (1, 2, 3, 4, 5), "libfabber_models_spatial_noise.so"))
    _, coords = volume
    supp, y = supp_series(coords, seed=72)
    V = y.shape[1]
    params = [dict(name="amp", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
              dict(name="r", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG)]

    def config(name, **kw):
        return vbabi.build_config(vbabi.MODEL_PLUGIN, V, T_SUPP, device_model=name, dt=0.25, params=params, suppdata=supp,
                                  param_overrides={"amp": dict(type="M")}, max_iterations=5, need_f=True, **kw)
    mvn = hiplib.init_posterior_host(config("suppconv_sp"), y)
    lane_cfg, wave_cfg = config("suppconv_sp", init_mvn=mvn), config("suppconv_spw", init_mvn=mvn)
    assert hiplib.spatial_kernel_name(lane_cfg) == "spatial<suppconv_sp,2>" and hiplib.spatial_kernel_name(wave_cfg) == "spatial<suppconv_spw,wave>"
    sp = vbabi.SpatialHolder(coords)
    lane, wave = hiplib.run_spatial_host(lane_cfg, sp, y), hiplib.run_spatial_host(wave_cfg, sp, y)
    assert np.all(lane["status"] == 0) and np.array_equal(lane["status"], wave["status"])
    lane.setdefault("f_history_len", np.zeros(V, dtype=np.int32))
    r = parity.strict(lane_cfg, lane, wave, what="spatial<suppconv_spw,wave> against spatial<suppconv_sp,2>", check_f=True)
    print("suppconv_spw against suppconv_sp: err means %.3e cov %.3e F %.3e" % (r["err_means"], r["err_cov"], r["err_f"]))
    # the curves handed to the wrong voxels are far outside these bounds
    moved = hiplib.run_spatial_host(vbabi.build_config(vbabi.MODEL_PLUGIN, V, T_SUPP, device_model="suppconv_spw", dt=0.25, params=params,
                                                       suppdata=np.roll(supp, 1, axis=1), param_overrides={"amp": dict(type="M")},
                                                       max_iterations=5, need_f=True, init_mvn=mvn), sp, y)
    n = 3
    assert np.abs(moved["mvn"][n * (n + 1) // 2] - wave["mvn"][n * (n + 1) // 2]).max() > 1e-2 * np.abs(wave["mvn"][n * (n + 1) // 2]).max()


# ---- 6. through fabber_dorun ----------------------------------------------------------------------------------------------
def test_multiexp_spw_through_fabber_run_against_the_host_model_route(library):
    """num-exps=5 under method=spatialvb with a spatial prior on every parameter, two iterations (from the library's start,
    every rate at 1, the fit is ill-conditioned beyond that: tests/test_spatial_wide.py); means and posterior image within
    the bounds that test holds the same model to"""
    rng = np.random.default_rng(51)
    shape, T, dt = (6, 5, 4), 50, 0.01
    t = np.arange(T) * dt
    amp = 1.0 + 0.3 * (np.arange(shape[0])[:, None, None] > 2) + np.zeros(shape)
    series = sum(a * np.exp(-r * t) for a, r in zip([1.0, 0.8, 0.6, 0.4, 0.3], [0.5, 3.0, 12.0, 40.0, 150.0]))
    data = (amp[..., None] * series + rng.normal(0, 0.02, shape + (T,))).astype(np.float32)
    opts = {"model": "multiexp_spw", "num-exps": 5, "dt": dt, "noise": "white", "method": "spatialvb", "max-iterations": 2,
            "param-spatial-priors": "M+", "save-mean": True, "save-mvn": True}
    dev = fabber.run(data, opts, model_libs=[library])
    host = fabber.run(data, dict(opts, **{"host-model": True}), model_libs=[library])
    assert "with the body 'multiexp_spw' of its library, kernels spatial<multiexp_spw,wave>" in dev["log"]
    assert "the model is evaluated on the host" not in dev["log"]
    assert "the model is evaluated on the host" in host["log"] and "of its library" not in host["log"]
    names = ["%s%d" % (nm, i + 1) for i in range(5) for nm in ("amp", "r")]
    for k in names:
        print("%s: max difference %.3e" % (k, np.abs(dev["mean_" + k] - host["mean_" + k]).max()))
        assert np.allclose(dev["mean_" + k], host["mean_" + k], rtol=2e-5, atol=1e-5), k
    assert np.allclose(dev["finalMVN"], host["finalMVN"], rtol=1e-4, atol=1e-7)
    # the initial posterior is the host class's (amp1 = the first sample, about 3 against the default of 1): the library
    # has no kernel for it, and two iterations from another start end far outside the bounds above
    assert "the initial posterior comes from the body" not in dev["log"]
    voxelwise = fabber.run(data, dict({k: v for k, v in opts.items() if k != "param-spatial-priors"}, method="vb", convergence="maxits"),
                           model_libs=[library])
    assert max(np.abs(dev["mean_" + k] - voxelwise["mean_" + k]).max() for k in names) > 1e-3  # (the spatial prior did something)
