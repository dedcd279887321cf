"""Every built-in spatial kernel table that no other test launches, against the oracle's spatial loop.

The spatial engine compiles one kernel table per (model, parameter count, noise policy): its own unrolled loops over P,
its own triangular indexing, LDS and state-row layout, its own register allocation. The other test files reach the
tables beyond "white noise, one precision" through three models only (poly with P = 2, exp with P = 2, the four-regressor
design), always with the spatial prior on the first parameter. CASES below lists one entry per remaining combination
(DESIGN.md section 5.2 has the table of which file runs which instantiation); every entry states the kernel table it
expects and the test asserts it first, so a change of routing cannot turn a case into a test of another kernel.

The problems are the smallest at which these kernels can still go wrong: 106 voxels of a masked 6 x 5 x 4 grid (more
than one wavefront, no multiple of 64, voxels with missing neighbours), 25 timepoints (no multiple of any class count),
a prior of every kind on the parameters after the first, with and without the free energy. test_cases_are_valid_for_the_
oracle (no GPU) keeps them honest: the oracle fails no voxel and its two CPU builds leave two thirds of the base
tolerance to the device."""
import re

import numpy as np
import pytest

import oracle
import parity
from fabber_core_amd import hiplib, vbabi

gpu = pytest.mark.gpu
AR = vbabi.NOISE_AR1

# the noise settings, by the key the case table uses
NOISES = {
    "white": dict(),
    "12": dict(noise_pattern="12"), "123": dict(noise_pattern="123"), "1234": dict(noise_pattern="1234"),
    "12345": dict(noise_pattern="12345"), "12345678": dict(noise_pattern="12345678"),
    "ar": dict(noise=AR),
    "ar2none": dict(noise=AR, num_echoes=2, ar_cross_terms="none"), "ar2same": dict(noise=AR, num_echoes=2, ar_cross_terms="same"),
    "ar2dual": dict(noise=AR, num_echoes=2, ar_cross_terms="dual"),
}
# ... and the kernel family each of them must reach
FAMILY = {"white": "", "12": ",pattern2", "123": ",pattern4", "1234": ",pattern4", "12345": ",pattern8", "12345678": ",pattern8",
          "ar": ",ar1", "ar2none": ",ar2:2", "ar2same": ",ar2:3", "ar2dual": ",ar2:4"}

# ---------------------------------------------------------------------------------------------
# The case table: (kernel table, noise setting, options). The model and the parameter count are read from the kernel's
# name. Options: T (series length, default 25; 26 under two echoes; 40 for the exponential model), masked (timepoints
# 2 and T - 1 are masked), image (an image prior in place of the N; where P has no N, in place of the last type).
# ---------------------------------------------------------------------------------------------
CASES = [
    # -- noise patterns with 2 and with 3 or 4 precisions, AR(1) with one echo --
    ("spatial<linear,1,pattern2>", "12", {}), ("spatial<linear,1,pattern4>", "123", {}), ("spatial<linear,1,ar1>", "ar", {}),
    ("spatial<linear,2,pattern2>", "12", {}), ("spatial<linear,2,pattern4>", "1234", {}), ("spatial<linear,2,ar1>", "ar", {}),
    ("spatial<linear,3,pattern2>", "12", {}), ("spatial<linear,3,pattern4>", "123", {}), ("spatial<linear,3,ar1>", "ar", {}),
    ("spatial<linear,5,pattern2>", "12", {}), ("spatial<linear,5,pattern4>", "1234", {}), ("spatial<linear,5,ar1>", "ar", {}),
    ("spatial<linear,6,pattern2>", "12", {}), ("spatial<linear,6,pattern4>", "123", {}), ("spatial<linear,6,ar1>", "ar", {}),
    ("spatial<poly,1,pattern2>", "12", {}), ("spatial<poly,1,pattern4>", "1234", {}), ("spatial<poly,1,ar1>", "ar", {}),
    ("spatial<poly,3,pattern2>", "12", {}), ("spatial<poly,3,pattern4>", "123", {}), ("spatial<poly,3,ar1>", "ar", {}),
    ("spatial<poly,4,pattern2>", "12", {}), ("spatial<poly,4,pattern4>", "1234", {}), ("spatial<poly,4,ar1>", "ar", {}),
    ("spatial<exp,4,pattern2>", "12", {}), ("spatial<exp,4,pattern4>", "123", {}), ("spatial<exp,4,pattern4>", "1234", {}),
    ("spatial<exp,4,ar1>", "ar", {}),
    #    an image prior, a short series, masked timepoints
    ("spatial<linear,6,pattern2>", "12", dict(image=True)), ("spatial<linear,6,pattern4>", "123", dict(image=True)),
    ("spatial<linear,6,ar1>", "ar", dict(image=True)),
    ("spatial<linear,3,pattern2>", "12", dict(T=10)), ("spatial<poly,3,pattern4>", "1234", dict(T=10)), ("spatial<poly,4,ar1>", "ar", dict(T=10)),
    ("spatial<linear,5,pattern2>", "12", dict(masked=True)), ("spatial<linear,2,pattern4>", "123", dict(masked=True)),
    ("spatial<poly,4,pattern2>", "12", dict(T=10, masked=True)),
    # -- noise patterns with 5 to 8 precisions --
    ("spatial<linear,1,pattern8>", "12345", {}), ("spatial<linear,1,pattern8>", "12345678", {}),
    ("spatial<linear,2,pattern8>", "12345", {}), ("spatial<linear,2,pattern8>", "12345678", {}),
    ("spatial<linear,3,pattern8>", "12345", {}), ("spatial<linear,3,pattern8>", "12345678", {}),
    ("spatial<linear,4,pattern8>", "12345", {}), ("spatial<linear,4,pattern8>", "12345678", {}),
    ("spatial<poly,1,pattern8>", "12345", {}), ("spatial<poly,1,pattern8>", "12345678", {}),
    ("spatial<poly,3,pattern8>", "12345", {}), ("spatial<poly,3,pattern8>", "12345678", {}),
    ("spatial<exp,2,pattern8>", "12345", {}), ("spatial<exp,2,pattern8>", "12345678", {}),
    ("spatial<exp,4,pattern8>", "12345", {}), ("spatial<exp,4,pattern8>", "12345678", {}),
    ("spatial<linear,4,pattern8>", "12345678", dict(image=True)),
    ("spatial<linear,3,pattern8>", "12345678", dict(T=10)),  # (six of the eight classes hold a single sample)
    ("spatial<poly,3,pattern8>", "12345", dict(masked=True)),
    # -- AR(1) with two echoes: 2, 3 and 4 AR coefficients --
    ("spatial<linear,2,ar2:2>", "ar2none", {}), ("spatial<linear,2,ar2:3>", "ar2same", {}), ("spatial<linear,2,ar2:4>", "ar2dual", {}),
    ("spatial<linear,3,ar2:2>", "ar2none", {}), ("spatial<linear,3,ar2:3>", "ar2same", {}), ("spatial<linear,3,ar2:4>", "ar2dual", {}),
    ("spatial<poly,3,ar2:2>", "ar2none", {}), ("spatial<poly,3,ar2:3>", "ar2same", {}), ("spatial<poly,3,ar2:4>", "ar2dual", {}),
    ("spatial<exp,4,ar2:2>", "ar2none", {}), ("spatial<exp,4,ar2:3>", "ar2same", {}), ("spatial<exp,4,ar2:4>", "ar2dual", {}),
    ("spatial<linear,3,ar2:3>", "ar2same", dict(image=True)),
    ("spatial<linear,2,ar2:4>", "ar2dual", dict(T=10)),
    # -- white noise with one precision --
    ("spatial<linear,1>", "white", {}), ("spatial<linear,2>", "white", {}), ("spatial<linear,3>", "white", {}),
    ("spatial<linear,4>", "white", {}), ("spatial<linear,5>", "white", {}), ("spatial<linear,6>", "white", {}),
    ("spatial<linear,8>", "white", {}), ("spatial<poly,4>", "white", {}), ("spatial<poly,6>", "white", {}),
    ("spatial<linear,8>", "white", dict(image=True)), ("spatial<linear,5>", "white", dict(T=10)),
    ("spatial<linear,6>", "white", dict(masked=True)), ("spatial<poly,4>", "white", dict(T=10, masked=True)),
]
# the tables of the models evaluated on the host (hiplib.run_spatial_hostmodel_host with the exact linearisation of the
# linear problems above, against the oracle's run of the built-in linear model)
HOST_CASES = [
    ("spatial<host,1,pattern2>", "12", {}), ("spatial<host,1,pattern4>", "1234", {}), ("spatial<host,1,ar1>", "ar", {}),
    ("spatial<host,3,pattern2>", "12", {}), ("spatial<host,3,pattern4>", "123", {}), ("spatial<host,3,ar1>", "ar", {}),
    ("spatial<host,4,pattern2>", "12", {}), ("spatial<host,4,pattern4>", "1234", {}), ("spatial<host,4,ar1>", "ar", {}),
    ("spatial<host,5,pattern2>", "12", {}), ("spatial<host,5,pattern4>", "123", {}), ("spatial<host,5,ar1>", "ar", {}),
    ("spatial<host,6,pattern2>", "12", {}), ("spatial<host,6,pattern4>", "1234", {}), ("spatial<host,6,ar1>", "ar", {}),
    ("spatial<host,6,pattern4>", "123", dict(image=True)), ("spatial<host,5,pattern2>", "12", dict(T=10, masked=True)),
    ("spatial<host,4,ar1>", "ar", dict(T=10)),
]

PRIOR_TYPES = ["M", "m", "P", "p", "A", "N", "M", "N"]  # by parameter position, cut to P
EXP4_MEANS = np.log([1.0, 0.7, 0.6, 6.0])  # amplitude, rate, amplitude, rate


def case_id(case):
    kernel, noise, opt = case
    return "-".join([kernel[len("spatial<"):-1], noise] + ["%s%s" % (k, "" if v is True else v) for k, v in sorted(opt.items())])


def parse_kernel(kernel):
    m = re.fullmatch(r"spatial<(linear|poly|exp|host),(\d+)((?:,[a-z0-9:]+)?)>", kernel)
    assert m, kernel
    return m.group(1), int(m.group(2)), m.group(3)


# ---------------------------------------------------------------------------------------------
# Problems
# ---------------------------------------------------------------------------------------------
def volume():
    rng = np.random.default_rng(3)
    mask = rng.random((6, 5, 4)) < 0.85
    coords = vbabi.grid_coords((6, 5, 4), mask)
    assert coords.shape[1] == 106
    return coords


def smooth_field(coords):
    return 1.0 + 0.3 * np.sin(coords[0] / 2.0) * np.cos(coords[1] / 3.0) + 0.1 * coords[2]


def ar_noise(T, V, rho, sd, seed):
    rng = np.random.default_rng(seed)
    e = rng.normal(0, sd, (T, V))
    for t in range(1, T):
        e[t] += rho * e[t - 1]
    return e


def cosine_design(T, P):
    t = np.arange(T)
    return np.cos(np.pi * (t[:, None] + 0.5) * np.arange(P)[None, :] / T)


def series_length(model, noise, opt):
    if "T" in opt:
        return opt["T"]
    return 40 if model == "exp" else (26 if noise.startswith("ar2") else 25)


def linear_problem(case, need_f, model_code=None):
    """The linear and the polynomial entries: P regressors (cosines, or the monomials of (t + 1) / T), per-voxel
    coefficients N(0, 1) plus a field that is smooth in space, noise of standard deviation 0.2 (AR(1) with rho = 0.3
    under the AR policies). Returns (holder, spatial, series, the design the data were generated from)."""
    kernel, noise, opt = case
    model, P, _ = parse_kernel(kernel)
    coords = volume()
    V, T = coords.shape[1], series_length(model, noise, opt)
    X = cosine_design(T, P) if model != "poly" else ((np.arange(T)[:, None] + 1.0) / T) ** np.arange(P)[None, :]
    # (seeds of their own for the polynomial: at degree 5 the two CPU builds' worst voxel is 2.7e-7 to 4.7e-7 apart
    # whatever the seed - the design's conditioning - and the test below wants the draw to leave TOL_MEAN / 3)
    seed = (1000 if model == "poly" else 0) + P
    rng = np.random.default_rng(100 + seed)
    coef = rng.normal(0, 1, (P, V)) + smooth_field(coords)[None, :]
    y = X @ coef + ar_noise(T, V, 0.3 if noise.startswith("ar") else 0.0, 0.2, 200 + seed)
    types = PRIOR_TYPES[:P]
    if opt.get("image"):
        types[types.index("N") if "N" in types else P - 1] = "I"
    names = ["c%d" % k for k in range(P)] if model == "poly" else ["Parameter_%d" % (k + 1) for k in range(P)]
    overrides = {n: dict(type=t) for n, t in zip(names, types)}
    images = {}
    if "I" in types:
        k = types.index("I")
        overrides[names[k]] = dict(type="I", prec=4.0)
        images[names[k]] = 0.2 + 0.05 * np.cos(coords[0] / 2.0) * np.cos(coords[1] / 3.0)
    kw = dict(max_iterations=5, need_f=need_f, param_overrides=overrides, image_priors=images, **NOISES[noise])
    if opt.get("masked"):
        kw["masked_timepoints"] = (2, T - 1)
    if model == "poly":
        h = vbabi.build_config(vbabi.MODEL_POLY, V, T, degree=P - 1, **kw)
    else:
        h = vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, **kw)
    return h, vbabi.SpatialHolder(coords), y, X


def exp_problem(case, need_f):
    """The exponential entries. Two exponentials (P = 4): started from its default posterior - two equal rates - the
    fit is the chaotic one (two CPU builds are 1e-5 to 1e-3 apart after four iterations), so it starts from
    an image with separated rates instead: the oracle's image after one iteration under the case's own noise settings
    (the right noise rows for every policy, the AR coefficients among them) with the model block of the covariance
    set to 0.05 I, no model-noise covariance, and the means at the values the data were generated from; three
    iterations from there. One exponential (P = 2): the ordinary start."""
    kernel, noise, opt = case
    _, P, _ = parse_kernel(kernel)
    coords = volume()
    V, T = coords.shape[1], series_length("exp", noise, opt)
    dt = 2.0 / T
    t = np.arange(T) * dt
    amp, rate = np.exp(EXP4_MEANS[0::2])[:P // 2], np.exp(EXP4_MEANS[1::2])[:P // 2]
    clean = sum(a * np.exp(-r * t) for a, r in zip(amp, rate))
    y = clean[:, None] * smooth_field(coords)[None, :] + ar_noise(T, V, 0.3 if noise.startswith("ar") else 0.0, 0.02, 300 + P)
    kw = dict(num_exps=P // 2, dt=dt, need_f=need_f, param_overrides={"amp1": dict(type="M")}, **NOISES[noise])
    sp = vbabi.SpatialHolder(coords)
    if P == 2:
        return vbabi.build_config(vbabi.MODEL_EXP, V, T, max_iterations=5, **kw), sp, y
    first = vbabi.build_config(vbabi.MODEL_EXP, V, T, max_iterations=1, **kw)
    img = oracle.run_spatial(first, sp, y)["mvn"].copy()
    n = P + first.n_noise_outputs
    nCov = n * (n + 1) // 2
    for i in range(n):
        for j in range(min(i, P - 1) + 1):
            img[i * (i + 1) // 2 + j] = 0.05 if i == j else 0.0
    for i in range(P):
        img[nCov + i] = EXP4_MEANS[i]
    return vbabi.build_config(vbabi.MODEL_EXP, V, T, max_iterations=3, init_mvn=img, **kw), sp, y


def problem(case, need_f):
    model = parse_kernel(case[0])[0]
    return exp_problem(case, need_f) if model == "exp" else linear_problem(case, need_f)[:3]


def host_problem(case, need_f):
    """a linear problem for the host-model route: under AR(1) noise (hiplib.initial_mvn writes white noise only) both
    sides continue from the oracle's image after one iteration"""
    h, sp, y, X = linear_problem(case, need_f)
    if case[1] == "ar":
        first, _, _, _ = linear_problem(case, need_f)
        first.cfg.max_iterations = 1
        img = oracle.run_spatial(first, sp, y)["mvn"].copy()
        h.keep["init_mvn"] = img
        h.cfg.init_mvn = img.ctypes.data
    return h, sp, y, X


def cpu_builds(h, sp, y, floor_on_exp):
    out = [oracle.run_spatial(h, sp, y), oracle.run_spatial_fma(h, sp, y)]
    if floor_on_exp:
        # (the build whose exp has the device's accuracy class is one of the CPU builds - DESIGN 5.4)
        out.append(oracle.run_spatial_exp1ulp(h, sp, y))
    for r in out:
        r.setdefault("f_history_len", np.zeros(h.cfg.n_voxels, dtype=np.int32))
    return out


def may_use_the_floor(case):
    """the exponential model (as tests/test_spatial_noise.py) and the polynomial of degree 5 (monomials up to t^5, as the
    degree-4 case of tests/test_spatial.py): DESIGN 5.2 lists them among the tests that opt in"""
    model, P, _ = parse_kernel(case[0])
    return model == "exp" or (model == "poly" and P == 6)


# ---------------------------------------------------------------------------------------------
# CPU: the table itself, and the cases as problems for the oracle
# ---------------------------------------------------------------------------------------------
def test_case_table_names_the_family_of_its_noise_setting():
    """every entry's kernel name carries the family of the noise setting it is run with, the pattern families are
    reached with every class count the issue names, and no entry appears twice"""
    for kernel, noise, opt in CASES + HOST_CASES:
        assert parse_kernel(kernel)[2] == FAMILY[noise], (kernel, noise)
        assert set(opt) <= {"T", "masked", "image"}
        assert not (opt.get("masked") and noise.startswith("ar"))  # (the AR policies refuse masked timepoints)
    ids = [case_id(c) for c in CASES + HOST_CASES]
    assert len(set(ids)) == len(ids)
    assert {n for _, n, _ in CASES} == set(NOISES)


def test_cases_are_valid_for_the_oracle():
    """(CPU) for every entry: the oracle fails no voxel, its CPU builds take the same iteration counts, and for the
    linear and polynomial entries the two builds agree within a third of the base tolerances - the reference alone
    leaves room under the bound the device is held to"""
    for case in CASES + HOST_CASES:
        for need_f in (False, True):
            what = "%s F=%d" % (case_id(case), need_f)
            model = parse_kernel(case[0])[0]
            if model == "host":
                h, sp, y, _ = host_problem(case, need_f)
            else:
                h, sp, y = problem(case, need_f)
            cpu = cpu_builds(h, sp, y, model == "exp")
            for r in cpu:
                assert np.all(r["status"] == 0) and np.isfinite(r["mvn"]).all(), what
                assert np.array_equal(r["iterations"], cpu[0]["iterations"]), what
            e_mean, e_cov, _ = parity.voxel_errors(h, cpu[0], cpu[1])
            if model != "exp":
                assert e_mean.max() < parity.TOL_MEAN / 3 and e_cov.max() < parity.TOL_COV / 3, (what, e_mean.max(), e_cov.max())
            if need_f:
                assert np.isfinite(cpu[0]["free_energy"]).all(), what


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def report(case, need_f, r):
    print("[instantiation] %s %s F=%d: means %.2e cov %.2e F %.2e%s"
          % (case[0], case_id(case), need_f, r["err_means"], r["err_cov"], r["err_f"], " (raised)" if r["raised"] else ""))


@gpu
@pytest.mark.parametrize("need_f", [False, True], ids=["noF", "F"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_builtin_instantiation_against_the_oracle(case, need_f):
    h, sp, y = problem(case, need_f)
    assert hiplib.spatial_kernel_name(h) == case[0]
    floor = may_use_the_floor(case)
    cpu = cpu_builds(h, sp, y, floor and h.cfg.model == vbabi.MODEL_EXP)
    got = hiplib.run_spatial_host(h, sp, y)
    kw = dict(allow_floor=True) if floor else {}
    r = parity.strict(h, cpu[0], got, what="%s F=%d" % (case_id(case), need_f), cpu2=cpu[1:], **kw)
    report(case, need_f, r)
    assert np.all(got["status"] == 0)
    assert floor or not r["raised"]


@gpu
@pytest.mark.parametrize("need_f", [False, True], ids=["noF", "F"])
@pytest.mark.parametrize("case", HOST_CASES, ids=case_id)
def test_host_model_instantiation_against_the_oracle(case, need_f):
    h, sp, y, X = host_problem(case, need_f)
    saved = (h.cfg.model, h.cfg.design)
    h.cfg.model, h.cfg.design = vbabi.MODEL_HOSTJAC, None  # (what run_spatial_hostmodel_host runs the configuration as)
    try:
        assert hiplib.spatial_kernel_name(h) == case[0]
    finally:
        h.cfg.model, h.cfg.design = saved
    cpu = cpu_builds(h, sp, y, False)
    got = hiplib.run_spatial_hostmodel_host(h, sp, y, lambda m, ids: (m @ X.T, X))
    r = parity.strict(h, cpu[0], got, what="%s F=%d" % (case_id(case), need_f), cpu2=cpu[1:])
    report(case, need_f, r)
    assert np.all(got["status"] == 0)
    assert not r["raised"]
