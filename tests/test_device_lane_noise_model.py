"""Lane-per-voxel kernels under AR(1) noise and noise patterns around the device body of a model library
(include/fabber_device_lane_noise_model.h): the engine's lane_ar1 / lane_phis kernels compiled in the library's code object
around the library's evaluator, against the CPU oracle with the built-in kernel of the same family as the control, against
the wave-per-voxel kernels of the same body, and through fabber_dorun against the host-model route of the same library
(tests/plugins/fwdmodel_lane_noise_models.hip: multiexp_lanenz, invrec_lanenz).

The shapes are the smallest at which these kernels can go wrong: 197 voxels are three full wavefronts and five lanes, 21
timepoints are neither a multiple of the 4-sample tile group nor of the prefetch trip (invrec: 16, one inversion time
each); the `lane` variant forces the route at these sizes."""
import contextlib
import ctypes as C
import re

import numpy as np
import pytest

import cases
import device_lane_noise_lib
import device_model_lib
import oracle
import parity
from fabber_core_amd import fabber, hiplib, vbabi

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not device_model_lib.engine_built(), reason="engine not built")]

AR = dict(noise=vbabi.NOISE_AR1, num_echoes=1)
PATTERN = dict(noise_pattern="12")
NOISES = {"ar1": AR, "pattern 12": PATTERN}
INVREC_KERNEL = {"ar1": "lane_ar1<invrec_lanenz,3,F>", "pattern 12": "lane_phis<invrec_lanenz,3,2>"}


@pytest.fixture(scope="module")
def library():
    assert hiplib.available() and hiplib.device_count() > 0
    path = device_lane_noise_lib.build_lane_noise_library()
    hiplib.load_model_library(path)
    assert device_lane_noise_lib.ENTRIES <= set(hiplib.device_lane_noise_models())
    return path


@contextlib.contextmanager
def variant(name):
    hiplib.set_variant(name)
    try:
        yield
    finally:
        hiplib.set_variant("auto")


# ---- multiexp_lanenz through the C ABI against the oracle's MODEL_EXP, the built-in kernel as the control ---------
def exp_pair(V, T, num_exps, dt, seed, f64=False, **opts):
    """tests/test_device_model.py::exp_pair with this library's body: the same problem for the oracle and the built-in
    kernel (the exponential model) and for the library's kernels, the initial image of the noise model included"""
    from test_device_model import initial_mvn
    ref, y = cases.exp_problem(V, T, num_exps, dt, seed=seed, **opts)
    if f64:
        y = y.astype(np.float64) + 1e-9  # (not representable in float32)
    mvn = initial_mvn(ref, y)
    ref, _ = cases.exp_problem(V, T, num_exps, dt, seed=seed, init_mvn=mvn, **opts)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="multiexp_lanenz", num_exps=num_exps, dt=dt, init_mvn=mvn,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num_exps), **opts)
    return ref, dev, y


# (options, float64 series, the family's kernel: lane_ar1<%s,2...> / lane_phis<%s,2,N> of the library and of the built-in model)
EXP_CASES = {
    "ar1": (dict(**AR), False, "lane_ar1<%s,2>"),
    "ar1,F": (dict(need_f=True, **AR), False, "lane_ar1<%s,2,F>"),
    "ar1,F watched": (dict(need_f=True, convergence="trialmode", **AR), False, "lane_ar1<%s,2,F>"),  # save buffer
    "ar1,F float64": (dict(need_f=True, **AR), True, "lane_ar1<%s,2,F>"),  # double tiles
    "pattern 12,F": (dict(noise_pattern="12", need_f=True), False, "lane_phis<%s,2,2>"),
    "pattern 123,F": (dict(noise_pattern="123", need_f=True), False, "lane_phis<%s,2,4>"),  # three of the four moment sets
    "pattern 1234,F watched": (dict(noise_pattern="1234", need_f=True, convergence="trialmode"), False, "lane_phis<%s,2,4>"),
    "pattern 12 masked": (dict(noise_pattern="12", masked_timepoints=(5,)), False, "lane_phis<%s,2,2>"),
}


@pytest.mark.parametrize("case", sorted(EXP_CASES))
def test_multiexp_lanenz_against_the_oracle(library, case):
    """The body computes the expression of the built-in exponential model, pointwise as the oracle does. Held to
    parity.strict at its base tolerances with status and iteration counts equal; the control is the built-in kernel of the
    same family on the same problem: the library's kernel gets a raised floor only where that one needs it, and its
    means stay within the bound tests/test_ar_noise.py applies to the built-in lane kernels."""
    opts, f64, kernel = EXP_CASES[case]
    ref, dev, y = exp_pair(197, 21, 1, 0.04, seed=20260102, f64=f64, max_iterations=10, **opts)
    cpu, cpu2 = oracle.run(ref, y), oracle.run_fma(ref, y)
    assert np.all(cpu["status"] == 0)
    with variant("lane"):
        assert hiplib.kernel_name(dev) == kernel % "multiexp_lanenz" and hiplib.kernel_name(ref) == kernel % "exp"
        got, builtin = hiplib.run_host(dev, y), hiplib.run_host(ref, y)
    r_builtin = parity.strict(ref, cpu, builtin, what=kernel % "exp" + " " + case, cpu2=cpu2, allow_floor=True)
    print("%s %s: err means %.3e rel %.3e cov %.3e F %.3e raised %s"
          % (kernel % "exp", case, r_builtin["err_means"], r_builtin["rel_means"], r_builtin["err_cov"], r_builtin["err_f"], r_builtin["raised"]))
    r = parity.strict(ref, cpu, got, what=kernel % "multiexp_lanenz" + " " + case, cpu2=cpu2, allow_floor=r_builtin["raised"])
    print("%s %s: err means %.3e rel %.3e cov %.3e F %.3e raised %s"
          % (kernel % "multiexp_lanenz", case, r["err_means"], r["rel_means"], r["err_cov"], r["err_f"], r["raised"]))
    assert r_builtin["raised"] or not r["raised"]
    assert r["rel_means"] < parity.NORTH_STAR or r["err_means"] < 1e-6


# ---- invrec_lanenz ---------------------------------------------------------------------------------------------------
TIS = np.linspace(0.1, 4.0, 16)
INVREC_PARAMS = [dict(name="M0", prior=(1.0, 1e6), post=(1.0, 1e6), prior_type="N", transform=vbabi.TRANSFORM_IDENTITY),
                 dict(name="T1", prior=(1.0, 100.0), post=(1.0, 1.5), prior_type="N", transform=vbabi.TRANSFORM_LOG),
                 dict(name="a", prior=(0.8, 4.0), post=(0.8, 1.0), prior_type="N", transform=vbabi.TRANSFORM_FRACTIONAL)]


def invrec_series(V, seed, noise_free=()):
    from test_device_lane_model import invrec_series as series
    return series(V, seed, noise_free=noise_free)[0]


def noise_image(h, white):
    """the initial posterior image of h's noise model from the one of white noise with one precision `white`: under AR(1)
    as Vb::BuildInitialMvn writes it (tests/test_device_model.py::initial_mvn: the alphas N(0, 1e4 I) first, then the
    precision); under a pattern hiplib.initial_mvn writes it itself"""
    cfg = h.cfg
    P, NA, N, V = cfg.n_params, 2 + cfg.ar_cross_terms, cfg.n_phis, cfg.n_voxels
    nw, n = P + 1, P + NA + N
    img = np.zeros((vbabi.mvn_rows(n), V))
    nCov = n * (n + 1) // 2
    for i in range(P):
        img[i * (i + 1) // 2 + i] = white[i * (i + 1) // 2 + i]
        img[nCov + i] = white[nw * (nw + 1) // 2 + i]
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


def invrec_problem(y, **opts):
    """through the C ABI: the initial posterior as the library's InitVoxelPosterior sets it (M0 = max |y|, of the finite
    samples: no route may start from NaN)"""
    V = y.shape[1]
    config = lambda **kw: vbabi.build_config(vbabi.MODEL_PLUGIN, V, len(TIS), device_model="invrec_lanenz", constants=TIS,
                                             params=INVREC_PARAMS, **kw)
    h = config(**opts)
    if h.cfg.noise == vbabi.NOISE_WHITE:
        mvn = hiplib.initial_mvn(h, y)
    else:
        mvn = noise_image(h, hiplib.initial_mvn(config(), y))
    n = h.cfg.n_params + h.n_noise_outputs
    mvn[n * (n + 1) // 2 + 0] = np.nanmax(np.abs(y.astype(np.float64)), axis=0)
    return config(init_mvn=mvn, **opts)


def lane_and_wave(h, y, kernel):
    with variant("lane"):
        assert hiplib.kernel_name(h) == kernel
        lane = hiplib.run_host(h, y)
    with variant("wave"):
        assert hiplib.kernel_name(h) == "wave<invrec_lanenz>"
        wave = hiplib.run_host(h, y)
    return lane, wave


def model_space_means(h, r):
    n = h.cfg.n_params + h.n_noise_outputs
    rows = r["mvn"][n * (n + 1) // 2:n * (n + 1) // 2 + h.cfg.n_params]
    return np.array([[vbabi.to_model(h.cfg.transform[i], float(x)) for x in rows[i]] for i in range(h.cfg.n_params)])


def differences(h, a, b, sel=None):
    """model-space means, the posterior image and F (relative: |F| > 1 is asserted) of a against b, each as a fraction of
    the caps of tests/test_device_lane_model.py::assert_results_agree: means rtol 2e-5 atol 1e-5, MVN rtol 1e-4 atol 1e-7,
    F rtol 1e-5"""
    sel = np.ones(h.cfg.n_voxels, dtype=bool) if sel is None else sel
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["iterations"], b["iterations"])
    assert np.abs(b["free_energy"][sel]).min() > 1.0, "F passes near zero: the relative comparison of F is ill-posed on this data"
    ma, mb = model_space_means(h, a)[:, sel], model_space_means(h, b)[:, sel]
    d_mean = np.max(np.abs(ma - mb) / (1e-5 + 2e-5 * np.abs(mb)))
    d_mvn = np.max(np.abs(a["mvn"][:, sel] - b["mvn"][:, sel]) / (1e-7 + 1e-4 * np.abs(b["mvn"][:, sel])))
    d_f = np.max(np.abs(a["free_energy"][sel] - b["free_energy"][sel]) / (1e-8 + 1e-5 * np.abs(b["free_energy"][sel])))
    return d_mean, d_mvn, d_f


def assert_results_agree(h, a, b, what, sel=None):
    d_mean, d_mvn, d_f = differences(h, a, b, sel)
    print("%s: lane against wave, as fractions of the caps (means rtol 2e-5 atol 1e-5, MVN rtol 1e-4 atol 1e-7, F rtol 1e-5): "
          "means %.3e MVN %.3e F %.3e" % (what, d_mean, d_mvn, d_f))
    assert d_mean <= 1 and d_mvn <= 1 and d_f <= 1


@pytest.mark.parametrize("noise", sorted(NOISES))
def test_invrec_lane_route_against_the_wave_route_of_the_same_body(library, noise):
    """... with four noise-free voxels: the moment form of k'Mk cancels there and the rescue pass evaluates the body,
    reading the constants. The caps are those of the white-noise lane kernels (tests/test_device_lane_model.py) and
    were not widened. Control, measured on an MI355X: the built-in exp model's lane against its wave kernel
    (set_variant) on problems of the same V, T, iterations and noise model (three seeds, noise 0.1 and 0.3) differ by at
    most 9.0e-4 / 9.3e-2 / 3.0e-3 of the caps on means / MVN / F under AR(1) and 1.3e-2 / 1.0e-1 / 1.3e-3 under pattern
    12 - the two routes differ in summation order only; this body's two routes by 3.0e-5 / 3.0e-3 / 1.5e-5 under AR(1)
    and 1.3e-5 / 2.2e-4 / 7.8e-4 under pattern 12."""
    noise_free = (3, 64, 130, 196)
    y = invrec_series(197, seed=51, noise_free=noise_free)
    h = invrec_problem(y, need_f=True, max_iterations=6, **NOISES[noise])
    lane, wave = lane_and_wave(h, y, INVREC_KERNEL[noise])
    assert np.all(wave["status"] == 0)
    assert_results_agree(h, lane, wave, noise)
    ml, mw = model_space_means(h, lane)[:, list(noise_free)], model_space_means(h, wave)[:, list(noise_free)]
    print("%s, noise-free voxels: max |d mean| %.3e" % (noise, np.max(np.abs(ml - mw))))


@pytest.mark.parametrize("noise", sorted(NOISES))
def test_last_partial_wavefront(library, noise):
    """voxel 64 of a run of 65 voxels (alone in its wavefront, 63 lanes repeating it) is bit for bit the voxel 64 of a
    run of 128"""
    y = invrec_series(128, seed=52)
    big = invrec_problem(y, need_f=True, max_iterations=6, **NOISES[noise])
    y65 = np.ascontiguousarray(y[:, :65])
    small = invrec_problem(y65, need_f=True, max_iterations=6, **NOISES[noise])
    with variant("lane"):
        assert hiplib.kernel_name(small) == INVREC_KERNEL[noise]
        a, b = hiplib.run_host(small, y65), hiplib.run_host(big, y)
    assert np.all(b["status"] == 0)
    for k in ("mvn", "free_energy", "status", "iterations"):
        assert np.array_equal(a[k][..., 64], b[k][..., 64]), k
        assert np.array_equal(a[k][..., :64], b[k][..., :64]), k


@pytest.mark.parametrize("noise", sorted(NOISES))
def test_a_failing_voxel_has_the_status_of_the_wave_route(library, noise):
    """a non-finite sample: that voxel alone carries the status the wave route gives it"""
    y = invrec_series(197, seed=55)
    y[5, 70] = np.nan
    h = invrec_problem(y, need_f=True, max_iterations=6, **NOISES[noise])
    lane, wave = lane_and_wave(h, y, INVREC_KERNEL[noise])
    assert wave["status"][70] != 0 and lane["status"][70] == wave["status"][70]
    assert lane["setup_failed"][70] == wave["setup_failed"][70]
    rest = np.ones(197, dtype=bool)
    rest[70] = False
    assert np.all(lane["status"][rest] == 0)
    assert_results_agree(h, lane, wave, noise + ", the other voxels", rest)


def test_blocks_of_the_host_entry_point_are_the_run_in_one(library, monkeypatch):
    """AR(1) with a detector that watches F: every block takes the lane kernel (the choice is made for the whole
    problem's voxel count), its save buffer - the larger one of the AR(1) kernels - comes from the block's slot, and the
    last block ends in a partial wavefront"""
    y = invrec_series(4096 + 37, seed=54)
    h = invrec_problem(y, need_f=True, convergence="trialmode", max_iterations=6, **AR)
    assert hiplib.kernel_name(h) == "lane_ar1<invrec_lanenz,3,F>"
    monkeypatch.setenv("FVB_HOST_BLOCK_VOXELS", "0")
    one = hiplib.run_host(h, y)
    monkeypatch.setenv("FVB_HOST_BLOCK_VOXELS", "1024")
    many = hiplib.run_host(h, y)
    for k in ("mvn", "free_energy", "status", "iterations"):
        assert np.array_equal(one[k], many[k]), k
    assert np.all(one["status"] == 0)


def test_device_pointers_run_the_lane_kernel(library):
    """DeviceProblem names the AR(1) lane kernel; the device entry point against the host entry point, bit for bit"""
    from fabber_core_amd.device import DeviceProblem
    y = invrec_series(4096, seed=57)
    h = invrec_problem(y, max_iterations=6, **AR)
    host = hiplib.run_host(h, y)
    prob = DeviceProblem(h, y, "cuda:0")
    assert prob.kernel == "lane_ar1<invrec_lanenz,3>"
    prob.run()
    dev = prob.results()
    assert np.array_equal(host["mvn"], dev["mvn"]) and np.array_equal(host["status"], dev["status"])
    assert np.all(host["status"] == 0)


@pytest.mark.parametrize("noise", sorted(NOISES))
def test_through_fabber_run_against_the_host_model_route(library, noise):
    """a 16 x 16 x 16 volume: 4096 voxels take the lane kernels without being asked to"""
    from test_device_model import assert_routes_agree
    y = invrec_series(4096, seed=53)
    data = y.T.reshape(16, 16, 16, len(TIS)).copy()
    opts = {"model": "invrec_lanenz", "method": "vb", "max-iterations": 6, "save-mean": True, "save-mvn": True, "save-free-energy": True}
    opts.update({"noise": "ar"} if noise == "ar1" else {"noise": "white", "noise-pattern": "12"})
    for i, ti in enumerate(TIS):
        opts["ti%d" % (i + 1)] = float(ti)
    dev = fabber.run(data, opts, model_libs=[library])
    host = fabber.run(data, dict(opts, **{"host-model": True}), model_libs=[library])
    assert "with the body 'invrec_lanenz' of its library" in dev["log"]
    assert "kernel %s, 4096 voxels x 16 timepoints" % INVREC_KERNEL[noise] in dev["log"]  # (F is saved: the AR(1) kernels with F)
    assert "evaluated on the host" in host["log"] and "of its library" not in host["log"]
    assert_routes_agree(dev, host, ("mean_M0", "mean_T1", "mean_a"))


# ---- the launcher's refusals -----------------------------------------------------------------------------------------
def launch(entry, family, pattern_n, feed, lds=0):
    """a hand-made call of a registered launcher with zeroed kernel arguments (no voxels, no F): (code, message)"""
    d = vbabi.FvbDeviceLaneNoiseModel(b"size_probe", vbabi.FVB_ABI_VERSION, 0, 3, vbabi.LANE_NOISE_AR1, 0, 0, 0, entry.launch)
    assert hiplib.lib().fabber_vb_register_device_lane_noise_model(C.byref(d)) == -72  # (the refusal states sizeof(KernelArgs))
    size =int(re.search(r"KernelArgs 0 against (\d+) bytes", hiplib.lib().fabber_vb_last_error().decode()).group(1))
    args, err = C.create_string_buffer(size), C.create_string_buffer(512)
    rc = entry.launch(C.cast(args, C.c_void_p), family, pattern_n, feed, lds, None, C.cast(err, C.c_void_p), len(err))
    return rc, err.value.decode()


def test_the_launcher_refuses_what_it_has_no_kernel_for(library):
    """a family outside the mask of the macro line, a feed the family has no kernel for: -40 with a message before anything
    is launched (a launch of these zeroed arguments - no voxels: an empty grid - would answer the launch error -100 - e)"""
    ar_only = hiplib.find_device_lane_noise_model("multiexp_lanenz", 4)
    assert ar_only.families == vbabi.LANE_NOISE_AR1
    assert ar_only.save_rows_ar1 > 0 and ar_only.save_rows_phis2 == 0 and ar_only.save_rows_phis4 == 0
    rc, msg = launch(ar_only, vbabi.LANE_NOISE_PHIS, 2, 0, lds=32)
    assert rc == -40 and "'multiexp_lanenz' with 4 parameters: not compiled with kernel family 2" in msg
    rc, msg = launch(ar_only, vbabi.LANE_NOISE_AR1, 0, 0)
    assert rc == -40 and "lane_ar1<multiexp_lanenz,4>: no instantiation for feed 0" in msg
    both = hiplib.find_device_lane_noise_model("invrec_lanenz", 3)
    assert both.families == vbabi.LANE_NOISE_AR1 | vbabi.LANE_NOISE_PHIS
    assert 0 < both.save_rows_phis2 < both.save_rows_phis4 and both.save_rows_ar1 > 0
    for feed in (1, 2):
        rc, msg = launch(both, vbabi.LANE_NOISE_PHIS, 2, feed, lds=32)
        assert rc == -40 and "lane_phis<invrec_lanenz,3,2>: no instantiation for feed %d" % feed in msg
    rc, msg = launch(both, vbabi.LANE_NOISE_PHIS, 3, 0, lds=32)  # (no kernel with three moment sets)
    assert rc == -40 and "lane_phis<invrec_lanenz,3,3>" in msg
    rc, msg = launch(both, 4, 0, 1)
    assert rc == -40 and "not compiled with kernel family 4" in msg
    assert hiplib.find_device_lane_noise_model("invrec_lanenz", 4) is None
