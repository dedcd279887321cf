"""Spatial VB around the device body of a model library (include/fabber_device_spatial_model.h): the engine's set-up
kernel and second sweep compiled in the library's code object around the library's evaluator, everything else of the
spatial family the engine's own - against the CPU oracle, the split first sweep against the per-level launches, and
through fabber_dorun against the host-model route of the same library (tests/plugins/fwdmodel_spatial_models.hip:
multiexp_sp, invrec_sp).

The shapes are the smallest at which these kernels can go wrong: a 7 x 6 x 5 volume masked to about 180 voxels has holes,
missing neighbours, five z-planes for the slab sweep, two full wavefronts and a partial one; 21 timepoints are no
multiple of the 8-timepoint trip."""
import numpy as np
import pytest

import oracle
import parity
import device_model_lib
from fabber_core_amd import fabber, hiplib, vbabi
from test_spatial import masked_volume, smooth_exp_data

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]

SHAPE, T, DT = (7, 6, 5), 21, 0.04


@pytest.fixture(scope="module")
def library():
    assert hiplib.available() and hiplib.device_count() > 0
    path = device_model_lib.build_spatial_library()
    hiplib.load_model_library(path)
    assert {("multiexp_sp", 2), ("multiexp_sp", 4), ("invrec_sp", 3)} <= set(hiplib.device_spatial_models())
    return path


@pytest.fixture(scope="module")
def volume():
    mask, coords = masked_volume(SHAPE, seed=61, keep=0.85)
    V = coords.shape[1]
    assert 128 < V < 192 and len(set(coords[2].tolist())) == 5
    return mask, coords


# ---- multiexp_sp through the C ABI against the oracle's MODEL_EXP ------------------------------------------------
def exp_data(coords, num_exps, seed):
    _, y = smooth_exp_data(coords, T, DT, seed=seed)
    if num_exps == 2:
        y = y + 0.5 * np.exp(-6.0 * np.arange(T) * DT)[:, None]
    return y.astype(np.float32)


def exp_pair(y, num_exps, **opts):
    """the same problem twice: for the oracle (and the built-in spatial kernels) as the exponential model, for the
    library's kernels as its body (same parameters, priors and initial posterior image)"""
    V = y.shape[1]
    ref = vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=num_exps, dt=DT, **opts)
    mvn = hiplib.initial_mvn(ref, y)
    ref = vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=num_exps, dt=DT, init_mvn=mvn, **opts)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_sp", num_exps=num_exps, dt=DT, init_mvn=mvn,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **opts)
    return ref, dev


def oracle_pair(ref, sp, y):
    cpu, cpu2 = oracle.run_spatial(ref, sp, y), oracle.run_spatial_fma(ref, sp, y)
    for r in (cpu, cpu2):
        r.setdefault("f_history_len", np.zeros(ref.cfg.n_voxels, dtype=np.int32))
    return cpu, cpu2


def library_against_builtin_against_oracle(ref, dev, sp, y, what, kernel, builtin_kernel, **kw):
    """parity.strict as spatial_check of tests/test_spatial.py applies it (status and iteration counts equal the
    oracle's), for the built-in kernels and for the library's on the same problem: the library's need no raised bound
    the built-in ones do not need"""
    assert hiplib.spatial_kernel_name(dev) == kernel and hiplib.spatial_kernel_name(ref) == builtin_kernel
    cpu, cpu2 = oracle_pair(ref, sp, y)
    builtin, lib = hiplib.run_spatial_host(ref, sp, y), hiplib.run_spatial_host(dev, sp, y)
    for name, got in ((builtin_kernel, builtin), (kernel, lib)):  # (the figures, before anything is asserted)
        ok = (cpu["status"] == 0) & (got["status"] == 0) & (cpu["iterations"] == got["iterations"])
        e_mean, e_cov, _ = parity.voxel_errors(ref, cpu, got, ok)
        print("%s %s: err means %.3e cov %.3e, status differs on %d voxels" % (name, what, e_mean.max(), e_cov.max(),
                                                                             np.count_nonzero(cpu["status"] != got["status"])))
    # the yardstick is measured, not judged here: tests/test_spatial.py holds the built-in kernels to the oracle. (On an
    # MI355X spatial<exp,2> is within the base tolerances in every case but prior type p, where it is at 1.29e-6 on the
    # means - base 1e-6, 3 x the distance of the two CPU builds 3.5e-8 - on this volume; the library's kernels are at
    # 3.1e-7 there.)
    try:
        builtin_raised = parity.strict(ref, cpu, builtin, what=builtin_kernel + " " + what, cpu2=cpu2, allow_floor=True, **kw)["raised"]
    except AssertionError as e:
        print("%s %s is outside parity.strict on this problem: %s" % (builtin_kernel, what, e.args[0]))
        builtin_raised = True
    r_lib = parity.strict(ref, cpu, lib, what=kernel + " " + what, cpu2=cpu2, allow_floor=True, **kw)
    print("%s %s: err means %.3e cov %.3e F %.3e raised %s (built-in: %s)" % (kernel, what, r_lib["err_means"], r_lib["err_cov"], r_lib["err_f"],
                                                                           r_lib["raised"], builtin_raised))
    assert builtin_raised or not r_lib["raised"]
    return cpu, lib


EXP_CASES = {
    "M": (dict(param_overrides={"amp1": dict(type="M")}), {}),
    "m": (dict(param_overrides={"amp1": dict(type="m")}), {}),
    "P": (dict(param_overrides={"amp1": dict(type="P")}), {}),
    "p": (dict(param_overrides={"amp1": dict(type="p")}), {}),
    "M next to ARD with F": (dict(need_f=True, param_overrides={"amp1": dict(type="M"), "r1": dict(type="A")}), dict(check_f=True)),
}


@pytest.mark.parametrize("case", sorted(EXP_CASES))
def test_multiexp_sp_against_the_oracle(library, volume, case):
    """The body computes the expression of the built-in exponential model, pointwise as the oracle does"""
    _, coords = volume
    opts, kw = EXP_CASES[case]
    y = exp_data(coords, 1, seed=62)
    ref, dev = exp_pair(y, 1, max_iterations=8, **opts)
    library_against_builtin_against_oracle(ref, dev, vbabi.SpatialHolder(coords), y, case, "spatial<multiexp_sp,2>", "spatial<exp,2>", **kw)


def test_biexponential_over_two_iterations(library, volume):
    """P = 4, two iterations only: the bi-exponential fit is chaotic over many"""
    _, coords = volume
    y = exp_data(coords, 2, seed=63)
    ref, dev = exp_pair(y, 2, max_iterations=2, need_f=True, param_overrides={"amp1": dict(type="M")})
    library_against_builtin_against_oracle(ref, dev, vbabi.SpatialHolder(coords), y, "two exponentials", "spatial<multiexp_sp,4>", "spatial<exp,4>",
                                           check_f=True)


# ---- the split first sweep ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["M with F", "two spatial parameters"])
def test_split_first_sweep_is_the_per_level_sweep_bit_for_bit(library, volume, case, monkeypatch):
    """the library's second sweep in the form that completes the split first sweep against its plain form after
    per-level launches, with the switches of the test of this name in tests/test_spatial.py"""
    _, coords = volume
    y = exp_data(coords, 1, seed=64)
    if case == "M with F":
        opts = dict(need_f=True, param_overrides={"amp1": dict(type="M")})
    else:
        opts = dict(param_overrides={"amp1": dict(type="M"), "r1": dict(type="m")})
    _, dev = exp_pair(y, 1, max_iterations=6, **opts)
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
            assert np.array_equal(split[k], per_level[k], equal_nan=True), (case, name, k)


# ---- failures ------------------------------------------------------------------------------------------------------
def test_a_failing_voxel_has_the_status_of_the_oracle_and_its_neighbours_carry_on(library, volume):
    """the construction of failing_voxel_problem (tests/test_spatial.py): a non-finite sample in two adjacent interior
    voxels and in the last one; with F it is caught before the voxel's means change, exactly those three fail"""
    _, coords = volume
    y = exp_data(coords, 1, seed=65)
    V = y.shape[1]
    bad = [V // 2, V // 2 + 1, V - 1]
    for v in bad:
        y[7, v] = np.nan
    ref, dev = exp_pair(y, 1, max_iterations=6, need_f=True, param_overrides={"amp1": dict(type="M")})
    # (the initial amplitude is max(y): of the finite samples, as in the oracle's own initial posterior nothing starts at NaN)
    n = 3
    for h in (ref, dev):
        h.keep["init_mvn"][n * (n + 1) // 2, bad] = np.nanmax(y[:, bad], axis=0)
    cpu, lib = library_against_builtin_against_oracle(ref, dev, vbabi.SpatialHolder(coords), y, "failing voxel", "spatial<multiexp_sp,2>",
                                                      "spatial<exp,2>", check_f=True)
    assert sorted(np.flatnonzero(cpu["status"]).tolist()) == sorted(bad)
    assert np.array_equal(lib["status"], cpu["status"])
    ok = lib["status"] == 0
    assert np.isfinite(lib["mvn"][:, ok]).all() and np.isfinite(lib["free_energy"][ok]).all()


TIS = np.linspace(0.1, 4.0, 16)
INVREC_PARAMS = [dict(name="M0", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
                 dict(name="T1", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG),
                 dict(name="a", prior=(0.8, 4.0), post=(0.8, 1.0), prior_type="N", transform=vbabi.TRANSFORM_FRACTIONAL)]


def invrec_series(coords, seed, noise_sd=2.0):
    """a smooth M0 of order 100 with noise of 2 (F stays away from zero)"""
    rng = np.random.default_rng(seed)
    V = coords.shape[1]
    m0 = 100.0 + 15.0 * np.sin(coords[0] / 2.0) * np.cos(coords[1] / 3.0)
    t1, a = rng.uniform(0.8, 1.6, V), rng.uniform(0.85, 0.98, V)
    clean = m0 * (1 - 2 * a * np.exp(-TIS[:, None] / t1))
    return (clean + rng.normal(0, noise_sd, clean.shape)).astype(np.float32)


def invrec_problem(y, constants=TIS, **opts):
    """through the C ABI: the initial posterior as the library's InitVoxelPosterior sets it (M0 = max |y|)"""
    V = y.shape[1]
    h = vbabi.build_config(vbabi.MODEL_PLUGIN, V, len(TIS), device_model="invrec_sp", constants=constants, params=INVREC_PARAMS, **opts)
    mvn = hiplib.initial_mvn(h, y)
    n = 4
    mvn[n * (n + 1) // 2 + 0] = np.abs(y.astype(np.float64)).max(axis=0)
    return vbabi.build_config(vbabi.MODEL_PLUGIN, V, len(TIS), device_model="invrec_sp", constants=constants, params=INVREC_PARAMS,
                              init_mvn=mvn, **opts)


def test_too_few_constants_stop_every_voxel_in_its_set_up(library, volume):
    """15 inversion times for 16 timepoints: the body answers the timepoint without a constant with a non-finite
    prediction - nothing is read past the constants block - and every voxel stops in the set-up kernel, with the status
    the wave kernels give it under voxelwise VB"""
    _, coords = volume
    y = invrec_series(coords, seed=66)
    spatial = invrec_problem(y, constants=TIS[:-1], max_iterations=3, param_overrides={"M0": dict(type="M")})
    assert hiplib.spatial_kernel_name(spatial) == "spatial<invrec_sp,3>"
    voxelwise = invrec_problem(y, constants=TIS[:-1], max_iterations=3)
    assert hiplib.kernel_name(voxelwise) == "wave<invrec_sp>"
    wave = hiplib.run_host(voxelwise, y)
    got = hiplib.run_spatial_host(spatial, vbabi.SpatialHolder(coords), y)
    assert np.all(wave["status"] == vbabi.STATUS_BAD_OFFSET) and np.all(wave["setup_failed"])
    assert np.array_equal(got["status"], wave["status"]) and np.array_equal(got["setup_failed"], wave["setup_failed"])
    # ... and with all of them the run is a run
    whole = hiplib.run_spatial_host(invrec_problem(y, max_iterations=3, param_overrides={"M0": dict(type="M")}), vbabi.SpatialHolder(coords), y)
    assert np.all(whole["status"] == 0) and np.isfinite(whole["mvn"]).all()


def test_a_missing_initial_posterior_is_refused_as_voxelwise_refuses_it(library, volume):
    _, coords = volume
    V = coords.shape[1]
    h = vbabi.build_config(vbabi.MODEL_PLUGIN, V, len(TIS), device_model="invrec_sp", constants=TIS, params=INVREC_PARAMS,
                           param_overrides={"M0": dict(type="M")})
    with pytest.raises(hiplib.HipEngineError, match="-52.*init_mvn"):
        hiplib.run_spatial_host(h, vbabi.SpatialHolder(coords), np.zeros((len(TIS), V), dtype=np.float32))


# ---- through fabber_dorun ------------------------------------------------------------------------------------------
def assert_routes_agree(dev, host, means, sel, fit_atol=1e-5):
    """the bounds tests/test_hostmodel.py holds the host route of spatial VB to against the device route of the same
    model: 2e-5 relative (atol 1e-5) on means, noise and model fit, the posterior image rtol 1e-4 atol 1e-7, F rtol 1e-5"""
    for k in tuple("mean_" + m for m in means) + ("noise_means",):
        print("%s: max relative difference %.3e" % (k, np.max(np.abs(host[k][sel] - dev[k][sel]) / np.abs(host[k][sel]))))
        assert host[k].dtype == np.float32 and np.allclose(host[k][sel], dev[k][sel], rtol=2e-5, atol=1e-5), k
    print("modelfit: max difference %.3e; finalMVN: max relative difference %.3e; freeEnergy: %.3e"
          % (np.max(np.abs(host["modelfit"][sel] - dev["modelfit"][sel])),
             np.max(np.abs(host["finalMVN"][sel] - dev["finalMVN"][sel]) / (1e-7 + np.abs(host["finalMVN"][sel]))),
             np.max(np.abs(host["freeEnergy"][sel] - dev["freeEnergy"][sel]) / np.abs(host["freeEnergy"][sel]))))
    assert np.allclose(host["modelfit"][sel], dev["modelfit"][sel], rtol=2e-5, atol=fit_atol)
    assert np.allclose(host["finalMVN"][sel], dev["finalMVN"][sel], rtol=1e-4, atol=1e-7)
    assert np.allclose(host["freeEnergy"][sel], dev["freeEnergy"][sel], rtol=1e-5)


def volume_of(coords, y):
    data = np.zeros(SHAPE + (y.shape[0],), dtype=np.float32)
    data[coords[0], coords[1], coords[2]] = y.T
    return data


SAVE = {"save-mean": True, "save-mvn": True, "save-free-energy": True, "save-noise-mean": True, "save-model-fit": True}


@pytest.mark.parametrize("model", ["multiexp_sp", "invrec_sp"])
def test_through_fabber_run_against_the_host_model_route(library, volume, model):
    mask, coords = volume
    if model == "multiexp_sp":
        y = exp_data(coords, 1, seed=67)
        opts = dict(SAVE, **{"model": model, "num-exps": 1, "dt": DT, "param-spatial-priors": "MN"})
        means, kernel, fit_atol = ("amp1", "r1"), "spatial<multiexp_sp,2>", 1e-5
    else:
        y = invrec_series(coords, seed=68)
        opts = dict(SAVE, **{"model": model, "param-spatial-priors": "MNN"})
        for i, ti in enumerate(TIS):
            opts["ti%d" % (i + 1)] = float(ti)
        # (both fits come from the host code, evaluated at means that agree to rtol 2e-5: on a curve of amplitude M0 that
        # passes through zero this is an absolute 2e-5 M0, as in tests/test_device_model.py)
        means, kernel, fit_atol = ("M0", "T1", "a"), "spatial<invrec_sp,3>", 2e-5 * float(np.abs(y).max())
    opts.update({"noise": "white", "method": "spatialvb", "max-iterations": 5})
    data = volume_of(coords, y)
    m = mask.astype(np.int32)
    dev = fabber.run(data, opts, mask=m, model_libs=[library])
    host = fabber.run(data, dict(opts, **{"host-model": True}), mask=m, model_libs=[library])
    assert "with the body '%s' of its library, kernels %s" % (model, kernel) in dev["log"]
    assert "evaluated on the host" not in dev["log"]
    assert "evaluated on the host" in host["log"] and "of its library" not in host["log"]
    assert_routes_agree(dev, host, means, mask, fit_atol)
    # the spatial prior did something: the fit differs from the voxelwise one
    plain = fabber.run(data, dict({k: v for k, v in opts.items() if k != "param-spatial-priors"}, method="vb"), mask=m, model_libs=[library])
    assert np.abs(plain["mean_" + means[0]][mask] - dev["mean_" + means[0]][mask]).max() > 1e-3 * float(np.abs(dev["mean_" + means[0]][mask]).max())


def test_ar_noise_keeps_the_host_route(library, volume):
    """no spatial kernels of a library body under AR(1) noise: the model's host code, with the log line of a model
    without kernels"""
    mask, coords = volume
    y = exp_data(coords, 1, seed=67)
    opts = {"model": "multiexp_sp", "num-exps": 1, "dt": DT, "param-spatial-priors": "MN", "noise": "ar", "method": "spatialvb",
            "max-iterations": 3, "save-mean": True}
    out = fabber.run(volume_of(coords, y), opts, mask=mask.astype(np.int32), model_libs=[library])
    assert "no device kernels for spatial VB" in out["log"] and "the model is evaluated on the host" in out["log"]
    assert "kernels spatial<" not in out["log"]
    assert np.isfinite(out["mean_amp1"][mask]).all()


# ---- device pointers -----------------------------------------------------------------------------------------------
def test_device_pointers_run_the_same_kernels(library, volume):
    """DeviceProblem.run_spatial (fabber_vb_run_spatial_device) with the constants block and the initial posterior on
    the device: the host entry point's result, bit for bit"""
    from fabber_core_amd.device import DeviceProblem
    _, coords = volume
    y = invrec_series(coords, seed=69)
    h = invrec_problem(y, max_iterations=5, need_f=True, param_overrides={"M0": dict(type="M")})
    sp = vbabi.SpatialHolder(coords)
    host = hiplib.run_spatial_host(h, sp, y)
    prob = DeviceProblem(h, y, "cuda:0")
    prob.run_spatial(sp)
    dev = prob.results()
    assert np.all(host["status"] == 0)
    for k in ("mvn", "status", "iterations", "free_energy"):
        assert np.array_equal(host[k], dev[k]), k
