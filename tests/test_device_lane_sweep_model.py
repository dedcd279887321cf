"""A sweep supplied by a model library's device body (the optional `template <int P> struct Sweep` of
include/fabber_device_lane_model.h, adapted by fvb::LibrarySweep): the lane kernels of every family linearise through it.
tests/plugins/fwdmodel_sweep_models.hip brings multiexp_sw, whose sweep restates the recurrence of the built-in exponential
model, and multiexp_swchk, whose sweep also checks the order contract and answers NaN when it is broken.

  - without a GPU: what the trait detects and that a body without a sweep keeps the pointwise sweep TYPE (so its kernels
    are compiled from the code they were compiled from before);
  - against the CPU oracle, with the built-in kernel of the same problem - the same arithmetic - as the yardstick;
  - against the wave route of the same body and against the pointwise body multiexp_lane;
  - the order contract for every series length around the 8-timepoint trip and its pipelined pair, on every feed;
  - AR(1), noise patterns, spatial VB; the last partial wavefront; fabber.run against the host-model route.

The shapes are the smallest at which this can go wrong: 197 voxels are three full wavefronts and five lanes; T runs over
{1, 7, 8, 9, 16, 17, 24, 25} for the contract and is 21 for the parity cases (neither a multiple of the trip nor of the
4-sample tile group); the `lane` variant forces the kernels at these sizes."""
import contextlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cases
import device_model_lib
import device_sweep_lib
import oracle
import parity
from fabber_core_amd import fabber, hiplib, vbabi

gpu = [pytest.mark.gpu, pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]


def on_gpu(f):
    for m in gpu:
        f = m(f)
    return f


# ---- without a GPU: the trait and the type of the sweep ---------------------------------------------------------------
STATIC_SOURCE = r"""
#include "fabber_device_lane_model.h"
namespace
{
struct Plain
{
    static __device__ __forceinline__ double eval(const fvb::ModelArgs &, int, int, const double *p)
    {
        return p[0];
    }
};
struct WithSweep : Plain
{
    template <int P>
    struct Sweep
    {
        __device__ __forceinline__ void init(const fvb::ModelArgs &, const double (&)[P], const double (&)[P], const double (&)[P])
        {
        }
        __device__ __forceinline__ void step(const fvb::ModelArgs &, int, bool, const double (&p)[P], const double (&p2)[P],
            const double (&p3)[P], double &g, double (&f2)[P], double (&f3)[P])
        {
            g = p[0];
            for (int i = 0; i < P; i++)
            {
                f2[i] = i == 0 ? p2[0] : p[0];
                f3[i] = i == 0 ? p3[0] : p[0];
            }
        }
    };
};
}
static_assert(fvb::body_has_sweep<WithSweep, 3>::value, "a body with Sweep is detected");
static_assert(!fvb::body_has_sweep<Plain, 3>::value, "a body without one is not");
static_assert(std::is_same<fvb::LibraryLane<Plain>::Model<3>::Sweep, fvb::PointwiseSweep<fvb::LibraryLane<Plain>::Model<3>, 3>>::value,
    "a body without a sweep keeps the pointwise sweep: the type of before");
static_assert(std::is_same<fvb::LibraryLane<WithSweep>::Model<3>::Sweep, fvb::LibrarySweep<WithSweep, 3>>::value,
    "a body with a sweep is linearised through the adapter");
"""


def test_the_trait_and_the_sweep_type_of_a_body_without_one():
    """hipcc -c for gfx950 of a few lines of static_asserts (no kernel is instantiated: a few seconds)"""
    with tempfile.TemporaryDirectory(prefix="sweep_static_") as tmp:
        src = os.path.join(tmp, "static_check.hip")
        with open(src, "w") as fh:
            fh.write(STATIC_SOURCE)
        p = subprocess.run([device_model_lib.hipcc()] + device_model_lib.HIP_FLAGS + device_model_lib.INCLUDES
                           + ["-c", src, "-o", os.path.join(tmp, "static_check.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]


# ---- on the GPU -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library():
    assert hiplib.available() and hiplib.device_count() > 0
    path = device_sweep_lib.build_sweep_library()
    hiplib.load_model_library(path)
    assert device_sweep_lib.LANE_ENTRIES <= set(hiplib.device_lane_models())
    assert device_sweep_lib.LANE_NOISE_ENTRIES <= set(hiplib.device_lane_noise_models())
    assert ("multiexp_sw", 2) in set(hiplib.device_spatial_models()) and ("multiexp_sw", 2) in set(hiplib.device_spatial_noise_models())
    return path


@pytest.fixture(scope="module")
def pointwise_library():
    """multiexp_lane of tests/plugins/fwdmodel_lane_models.hip: the same eval, no sweep"""
    path = device_model_lib.build_lane_library()
    hiplib.load_model_library(path)
    return path


@contextlib.contextmanager
def variant(name):
    hiplib.set_variant(name)
    try:
        yield
    finally:
        hiplib.set_variant("auto")


def exp_problems(V, T, num_exps, dt, seed, models=("multiexp_sw",), f64=False, noise_free=(), noise_sd=0.1, **opts):
    """the same problem for the oracle and the built-in kernel (the exponential model) and for every body of `models`
    (same parameters, priors and initial posterior image, the noise model's block included): ref, {model: holder}, y"""
    from test_device_model import initial_mvn
    ref, y = cases.exp_problem(V, T, num_exps, dt, seed=seed, noise_sd=noise_sd, **opts)
    if noise_free:  # (the moment form of k'k cancels there: the residual passes run)
        clean = cases.exp_problem(V, T, num_exps, dt, seed=seed, noise_sd=0.0, **opts)[1]
        y[:, list(noise_free)] = clean[:, list(noise_free)]
    if f64:
        y = y.astype(np.float64) + 1e-9  # (not representable in float32)
    mvn = initial_mvn(ref, y)
    ref, _ = cases.exp_problem(V, T, num_exps, dt, seed=seed, init_mvn=mvn, **opts)
    devs = {m: vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=m, num_exps=num_exps, dt=dt, init_mvn=mvn,
                                  params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **opts) for m in models}
    return ref, devs, y


def bit_identical(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("mvn", "free_energy", "status", "iterations"))


# ---- against the oracle, the built-in kernel as the yardstick -------------------------------------------------------------
def oracle_cases():
    from test_device_lane_model import EXP_CASES
    return EXP_CASES


@on_gpu
@pytest.mark.parametrize("case", ["F counted", "F watched", "float64", "float64 counted", "masked timepoint", "masked timepoint,F", "white"])
def test_multiexp_sw_against_the_oracle(library, case):
    """The cases of tests/test_device_lane_model.py. The yardstick is lane<exp,2> on the same problem, whose sweep has the
    arithmetic this body's sweep restates: a raised bound only where that kernel needs one, and an error on the means of
    at most twice that kernel's (two roundings' worth covers instruction scheduling; a missing resync would give far
    more)."""
    opts, f64, kernel = oracle_cases()[case]
    kernel = kernel.replace("multiexp_lane", "multiexp_sw")
    ref, devs, y = exp_problems(197, 21, 1, 0.04, seed=20260102, f64=f64, max_iterations=10, **opts)
    dev = devs["multiexp_sw"]
    cpu, cpu2 = oracle.run(ref, y), oracle.run_fma(ref, y)
    with variant("lane"):
        assert hiplib.kernel_name(dev) == kernel and hiplib.kernel_name(ref) == kernel.replace("multiexp_sw", "exp")
        got, builtin = hiplib.run_host(dev, y), hiplib.run_host(ref, y)
    r_builtin = parity.strict(ref, cpu, builtin, what="lane<exp,2> " + case, cpu2=cpu2, allow_floor=True)
    r = parity.strict(ref, cpu, got, what=kernel + " " + case, cpu2=cpu2, allow_floor=r_builtin["raised"])
    print("%s: err means built-in %.3e sweep %.3e (cov %.3e / %.3e, F %.3e / %.3e), raised %s / %s, posteriors bit-identical: %s"
          % (case, r_builtin["err_means"], r["err_means"], r_builtin["err_cov"], r["err_cov"], r_builtin["err_f"], r["err_f"],
             r_builtin["raised"], r["raised"], bit_identical(got, builtin)))
    assert r_builtin["raised"] or not r["raised"]
    assert r["err_means"] <= 2 * r_builtin["err_means"]


@on_gpu
def test_biexponential_needs_no_bound_the_builtin_kernel_does_not_need(library):
    """P = 4, two iterations (the bi-exponential fit is chaotic over many): lane<multiexp_sw,4> and the
    built-in lane<exp,4> on the same problem against the oracle"""
    ref, devs, y = exp_problems(197, 21, 2, 0.04, seed=20260103, max_iterations=2, need_f=True)
    dev = devs["multiexp_sw"]
    cpu, cpu2 = oracle.run(ref, y), oracle.run_fma(ref, y)
    with variant("lane"):
        assert hiplib.kernel_name(dev) == "lane<multiexp_sw,4,F>" and hiplib.kernel_name(ref) == "lane<exp,4,F>"
        lib, builtin = hiplib.run_host(dev, y), hiplib.run_host(ref, y)
    r_builtin = parity.strict(ref, cpu, builtin, what="lane<exp,4,F>", cpu2=cpu2, allow_floor=True)
    print("lane<exp,4,F>: err means %.3e cov %.3e F %.3e raised %s" % (r_builtin["err_means"], r_builtin["err_cov"], r_builtin["err_f"], r_builtin["raised"]))
    r_lib = parity.strict(ref, cpu, lib, what="lane<multiexp_sw,4,F>", cpu2=cpu2, allow_floor=True)
    print("lane<multiexp_sw,4,F>: err means %.3e cov %.3e F %.3e raised %s; bit-identical to the built-in: %s"
          % (r_lib["err_means"], r_lib["err_cov"], r_lib["err_f"], r_lib["raised"], bit_identical(lib, builtin)))
    assert r_builtin["raised"] or not r_lib["raised"]


# ---- against the other routes of the same body ---------------------------------------------------------------------------
def decay_series(shape, T, dt, seed, noise_sd=0.3):
    """amplitudes of 10 and 5, rates of 2 and 3, noise of 0.3 (float32, shape + (T,)): a series that determines its
    parameters. Comparisons of two ROUTES need that: with the amplitudes 1 and 0.5 and the noise of 0.3 of
    cases.exp_problem the mean of log r is still within 0.5 of zero after two iterations with a wide posterior, and every
    pair there is disagrees by more than the cap on the posterior image (absolute part 1e-7) - the parent's own
    lane<exp,2> and lane<multiexp_lane,2> by 2.0 times the cap, each of them and the CPU oracle by 6 to 8 times, measured
    on an MI355X. On this series those pairs are at 2e-3 and 3e-3 of the cap after two iterations, 5e-7 after ten, and
    |F| stays above 10 (assert_results_agree compares F relatively)."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) * dt
    amp = np.where(rng.random(shape) < 0.5, 10.0, 5.0)
    rate = np.where(rng.random(shape) < 0.5, 2.0, 3.0)
    return (amp[..., None] * np.exp(-rate[..., None] * t) + rng.normal(0, noise_sd, tuple(shape) + (T,))).astype(np.float32)


def routes_problem(max_iterations, models):
    """197 voxels x 21 timepoints of decay_series for every body of `models`: {model: holder}, y [T][V]"""
    V, T, dt = 197, 21, 0.04
    y = np.ascontiguousarray(decay_series((V,), T, dt, seed=20260104).T)
    opts = dict(need_f=True, max_iterations=max_iterations)
    mvn = hiplib.initial_mvn(vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=1, dt=dt, **opts), y)
    devs = {m: vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=m, num_exps=1, dt=dt, init_mvn=mvn,
                                  params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1), **opts) for m in models}
    return devs, y


@on_gpu
def test_lane_route_against_the_wave_route_of_the_same_body(library):
    """the lane kernels linearise through the sweep, the wave kernels through eval: the caps of
    tests/test_device_lane_model.py::assert_results_agree"""
    from test_device_lane_model import assert_results_agree
    devs, y = routes_problem(10, ("multiexp_sw",))
    h = devs["multiexp_sw"]
    with variant("lane"):
        assert hiplib.kernel_name(h) == "lane<multiexp_sw,2,F>"
        lane = hiplib.run_host(h, y)
    with variant("wave"):
        assert hiplib.kernel_name(h) == "wave<multiexp_sw>"
        wave = hiplib.run_host(h, y)
    assert np.all(wave["status"] == 0)
    assert_results_agree(h, lane, wave)


@on_gpu
@pytest.mark.parametrize("iterations", [2, 10])
def test_against_the_pointwise_body_on_the_same_problem(library, pointwise_library, iterations):
    """multiexp_lane has the same eval and no sweep. Two iterations are the precise passes alone: every step is exact.
    Over ten the recurrence runs: the results agree within the caps AND differ in their bits - the run-time evidence that
    the sweep is what the kernel evaluates."""
    from test_device_lane_model import assert_results_agree
    devs, y = routes_problem(iterations, ("multiexp_sw", "multiexp_lane"))
    with variant("lane"):
        assert hiplib.kernel_name(devs["multiexp_sw"]) == "lane<multiexp_sw,2,F>"
        assert hiplib.kernel_name(devs["multiexp_lane"]) == "lane<multiexp_lane,2,F>"
        sweep, pointwise = hiplib.run_host(devs["multiexp_sw"], y), hiplib.run_host(devs["multiexp_lane"], y)
    assert np.all(pointwise["status"] == 0)
    same = np.array_equal(sweep["mvn"], pointwise["mvn"])
    print("%d iterations: sweep body against pointwise body, posterior images bit-identical: %s" % (iterations, same))
    assert_results_agree(devs["multiexp_sw"], sweep, pointwise)
    if iterations == 10:
        assert not same


# ---- the order contract ---------------------------------------------------------------------------------------------------
SERIES_LENGTHS = (1, 7, 8, 9, 16, 17, 24, 25)
FEEDS = {
    "float tiles": (dict(), False, "lane<%s,2>"),
    "double tiles": (dict(), True, "lane<%s,2>"),
    "in place": (dict(masked_timepoints=(2,)), False, "lane<%s,2>"),
    "ar1": (dict(noise=vbabi.NOISE_AR1, num_echoes=1), False, "lane_ar1<%s,2>"),
    "pattern 12": (dict(noise_pattern="12"), False, "lane_phis<%s,2,2>"),
}
# (a noise pattern longer than the series is refused, as the reference refuses it, and a series of one timepoint has none
# to spare for the mask: these two feeds start at two timepoints)
CONTRACT_CASES = [(feed, T) for feed in sorted(FEEDS) for T in SERIES_LENGTHS if not (feed in ("pattern 12", "in place") and T < 2)]


@on_gpu
@pytest.mark.parametrize("feed,T", CONTRACT_CASES)
def test_the_order_contract_on_every_feed(library, feed, T):
    """multiexp_swchk answers a NaN g - the voxel stops with a non-zero status - from the step at which init had not come
    first, the first step was not exact, a timepoint came out of order or 8 steps had passed since an exact one. Ten
    iterations: the precise passes and the recurrence; four voxels without noise, where the moment form of the residual
    cancels and the passes that form a linearisation again run. Every voxel ends with status 0 and with multiexp_sw's
    means, bit for bit. (The masked timepoint of the in-place feed is the second one: a step that is not exact, and the
    sweep takes it like any other.)

    Bit for bit across two instantiations of a kernel holds where the compiler fuses the same products in both: the test
    library compiles its AR(1) / noise-pattern parts with contraction off outside the model code for that
    (tests/plugins/fwdmodel_sweep_models.hip says what was seen without: the last bit of a few voxels after two
    iterations, under AR(1) at T = 8, 9, 24, 25 only)."""
    opts, f64, kernel = FEEDS[feed]
    noise_free = (3, 64, 130, 196) if T > 2 else ()
    _, devs, y = exp_problems(197, T, 1, 0.04, seed=20260105 + T, models=("multiexp_sw", "multiexp_swchk"), f64=f64,
                              noise_free=noise_free, max_iterations=10, **opts)
    with variant("lane"):
        assert hiplib.kernel_name(devs["multiexp_swchk"]) == kernel % "multiexp_swchk" and hiplib.kernel_name(devs["multiexp_sw"]) == kernel % "multiexp_sw"
        checked, plain = hiplib.run_host(devs["multiexp_swchk"], y), hiplib.run_host(devs["multiexp_sw"], y)
    print("%s, T = %d: status counts checked %s plain %s" % (feed, T, np.unique(checked["status"], return_counts=True), np.unique(plain["status"], return_counts=True)))
    assert np.all(checked["status"] == 0)
    assert np.array_equal(checked["mvn"], plain["mvn"]) and np.array_equal(checked["iterations"], plain["iterations"])


# ---- the other lane families ------------------------------------------------------------------------------------------------
def noise_cases():
    from test_device_lane_noise_model import EXP_CASES
    return EXP_CASES


@on_gpu
@pytest.mark.parametrize("case", ["ar1", "ar1,F", "ar1,F float64", "ar1,F watched", "pattern 12 masked", "pattern 12,F"])
def test_multiexp_sw_under_ar1_and_pattern_12_against_the_oracle(library, case):
    """as tests/test_device_lane_noise_model.py holds multiexp_lanenz: parity.strict with status and iteration counts
    equal, the built-in kernel of the family as the control"""
    opts, f64, kernel = noise_cases()[case]
    ref, devs, y = exp_problems(197, 21, 1, 0.04, seed=20260102, f64=f64, max_iterations=10, **opts)
    dev = devs["multiexp_sw"]
    cpu, cpu2 = oracle.run(ref, y), oracle.run_fma(ref, y)
    assert np.all(cpu["status"] == 0)
    with variant("lane"):
        assert hiplib.kernel_name(dev) == kernel % "multiexp_sw" and hiplib.kernel_name(ref) == kernel % "exp"
        got, builtin = hiplib.run_host(dev, y), hiplib.run_host(ref, y)
    r_builtin = parity.strict(ref, cpu, builtin, what=kernel % "exp" + " " + case, cpu2=cpu2, allow_floor=True)
    r = parity.strict(ref, cpu, got, what=kernel % "multiexp_sw" + " " + case, cpu2=cpu2, allow_floor=r_builtin["raised"])
    print("%s: err means built-in %.3e sweep %.3e rel %.3e cov %.3e F %.3e, raised %s / %s, bit-identical to the built-in: %s"
          % (case, r_builtin["err_means"], r["err_means"], r["rel_means"], r["err_cov"], r["err_f"], r_builtin["raised"], r["raised"],
             bit_identical(got, builtin)))
    assert r_builtin["raised"] or not r["raised"]
    assert r["rel_means"] < parity.NORTH_STAR or r["err_means"] < 1e-6


@on_gpu
@pytest.mark.parametrize("noise", ["white", "ar1", "pattern 12"])
def test_spatial_vb_against_the_oracle(library, noise):
    """method=spatialvb on the masked volume of tests/test_device_spatial_model.py, prior M on the amplitude, under that
    file's conditions: no raised bound the built-in kernels do not need"""
    from test_device_spatial_model import DT, SHAPE, T, exp_data, library_against_builtin_against_oracle
    from test_device_model import initial_mvn
    from test_spatial import masked_volume
    _, coords = masked_volume(SHAPE, seed=61, keep=0.85)
    noise_opts, tag = {"white": ({}, ""), "ar1": (dict(noise=vbabi.NOISE_AR1, num_echoes=1), ",ar1"), "pattern 12": (dict(noise_pattern="12"), ",pattern2")}[noise]
    y = exp_data(coords, 1, seed=62)
    V = y.shape[1]
    opts = dict(max_iterations=8, param_overrides={"amp1": dict(type="M")}, **noise_opts)
    ref = vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=1, dt=DT, **opts)
    mvn = initial_mvn(ref, y)
    ref = vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=1, dt=DT, init_mvn=mvn, **opts)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_sw", num_exps=1, dt=DT, init_mvn=mvn,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1), **opts)
    library_against_builtin_against_oracle(ref, dev, vbabi.SpatialHolder(coords), y, "M, " + noise, "spatial<multiexp_sw,2%s>" % tag,
                                           "spatial<exp,2%s>" % tag)


# ---- unchanged neighbours ---------------------------------------------------------------------------------------------------
@on_gpu
def test_last_partial_wavefront(library):
    """voxel 64 of a run of 65 voxels (alone in its wavefront, 63 lanes repeating it) is bit for bit the voxel 64 of a
    run of 128"""
    _, big, y = exp_problems(128, 21, 1, 0.04, seed=20260106, need_f=True, max_iterations=10)
    _, small, y65 = exp_problems(128, 21, 1, 0.04, seed=20260106, need_f=True, max_iterations=10)
    y65 = np.ascontiguousarray(y65[:, :65])
    mvn65 = np.ascontiguousarray(small["multiexp_sw"].keep["init_mvn"][:, :65])
    small = vbabi.build_config(vbabi.MODEL_PLUGIN, 65, 21, device_model="multiexp_sw", num_exps=1, dt=0.04, init_mvn=mvn65, need_f=True,
                               max_iterations=10, params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=1))
    with variant("lane"):
        assert hiplib.kernel_name(small) == "lane<multiexp_sw,2,F>"
        a, b = hiplib.run_host(small, y65), hiplib.run_host(big["multiexp_sw"], y)
    assert np.all(b["status"] == 0)
    for k in ("mvn", "free_energy", "status", "iterations"):
        assert np.array_equal(a[k][..., 64], b[k][..., 64]), k
        assert np.array_equal(a[k][..., :64], b[k][..., :64]), k


@on_gpu
def test_through_fabber_run_against_the_host_model_route(library):
    """a 16 x 16 x 16 volume of decay_series: 4096 voxels take the lane kernels without being asked to (the oracle's F runs
    from -43 to -12 on this data, away from zero as tests/test_device_model.py::assert_routes_agree wants it)"""
    from test_device_model import assert_routes_agree
    data = decay_series((16, 16, 16), 40, 0.04, seed=20260107)
    opts = {"model": "multiexp_sw", "num-exps": 1, "dt": 0.04, "noise": "white", "method": "vb", "max-iterations": 6, "save-mean": True,
            "save-mvn": True, "save-free-energy": True}
    dev = fabber.run(data, opts, model_libs=[library])
    host = fabber.run(data, dict(opts, **{"host-model": True}), model_libs=[library])
    assert "with the body 'multiexp_sw' of its library" in dev["log"]
    assert "kernel lane<multiexp_sw,2,F>, 4096 voxels x 40 timepoints" in dev["log"]
    assert "evaluated on the host" in host["log"] and "of its library" not in host["log"]
    assert_routes_agree(dev, host, ("mean_amp1", "mean_r1"))
