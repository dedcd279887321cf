"""Every built-in lane-per-voxel kernel and every feed of it, against the oracle's voxelwise loop.

The lane engine compiles one kernel per (model, parameter count, noise family, F, feed): its own unrolled loops over P,
its own register allocation and spills, its own LDS parking plan, and above P = 4 another routine behind a cancelled
k'Qk. The other test files reach a handful of the names at the oracle's sizes and the rest only where the seeded
random sweep happens to draw them (DESIGN.md section 5.2 has the table of which file runs which instantiation). The
tables below hold one entry per name and per feed; every GPU case asserts hiplib.kernel_name first, under
hiplib.set_variant("lane"), so a change of routing cannot turn a case into a test of another kernel.

  1. NAMES     every compiled name once, float series, with and without F: fp32 tiles (the series in place for
               lane_phis), the counting instance where there is F
  2. FEEDS     the white-noise names again as float64 (fp64 tiles) and with two masked timepoints, the last among
               them (the series in place); WATCHING: one P per model and family with convergence=trialmode on a
               float64 series (the save buffer, the instance that watches F); lane_phis as float64 and masked
  3. LENGTHS   series lengths around the trip pipeline of the tiled feed: fewer than 8 timepoints, one to three trips,
               odd and even trip counts, every remainder mod 8 / 4 / 2, the 16-byte rounding of the pattern kernels'
               class bytes, the 64- and 128-timepoint strides of the fallbacks
  4. FORCED    hiplib.set_residual_tolerance(1.0): every voxel takes the direct sum behind a cancelled k'Qk in every
               iteration - which is what the reference always computes, so the oracle is still the reference - and
               the same problem with its voxels reversed returns the reversed result bit for bit (DESIGN 3.1 / 5.3:
               what a voxel gets depends on nothing but that voxel)
  5. EDGES     1, 63, 64, 65 and 257 voxels: strict parity, and the first V voxels of one 257-voxel run bit for bit

The problems are the smallest at which these kernels can still go wrong: 197 voxels (three full wavefronts and five
lanes, no multiple of the 256-thread grid that re-lays the series), 25 timepoints (26 under two echoes, 40 for the
exponential model), five iterations. test_cases_are_valid_for_the_oracle (no GPU) keeps them honest: the oracle fails
no voxel, its CPU builds take the same iteration counts, and outside the stated opt-ins (the polynomial with six
parameters - monomials up to t^5 - and the exponential model, whose floor includes the CPU build with a 1-ulp exp,
DESIGN 5.4) two CPU builds leave two thirds of the base tolerances to the device.

The polynomial with 7 and 8 parameters is NOT here: over 9, 12 and 25 timepoints two CPU builds of the oracle are 3e-4
to more than 1 apart after a single iteration (cond(J'J) > 1e16), so there is no value to compare and no bound that
could be derived from the reference. lane<poly,7> and lane<poly,8> stay with tests/test_hip_parity.py::
test_seven_and_eight_parameters_on_the_lane_kernel (dispatch and a finite result)."""
import functools
import re

import numpy as np
import pytest

import hipengine
import oracle
import parity
from fabber_core_amd import hiplib, vbabi

gpu = pytest.mark.gpu
AR = vbabi.NOISE_AR1
V_DEFAULT = 197
V_EDGE_FULL = 257

# the noise settings, by the key the case tables use ...
NOISES = {
    "white": dict(),
    "12": dict(noise_pattern="12"), "123": dict(noise_pattern="123"), "1234": dict(noise_pattern="1234"),
    "ar": dict(noise=AR),
    "ar2none": dict(noise=AR, num_echoes=2, ar_cross_terms="none"), "ar2same": dict(noise=AR, num_echoes=2, ar_cross_terms="same"),
    "ar2dual": dict(noise=AR, num_echoes=2, ar_cross_terms="dual"),
}
# ... and the kernel family (with its N or NA) each of them must reach
FAMILY = {"white": ("lane", None), "12": ("lane_phis", 2), "123": ("lane_phis", 4), "1234": ("lane_phis", 4), "ar": ("lane_ar1", None),
          "ar2none": ("lane_ar2", 2), "ar2same": ("lane_ar2", 3), "ar2dual": ("lane_ar2", 4)}

# Every name the lane engine compiles (FVB_LANE_CASE, FVB_LANE_PATTERN_CASE, FVB_LANE_AR_CASE, FVB_LANE_ARN_CASE in
# vb_lane_*.hip), literally: a new instantiation without a case below fails test_every_compiled_name_has_a_case.
COMPILED = """
lane<linear,1> lane<linear,2> lane<linear,3> lane<linear,4> lane<linear,5> lane<linear,6> lane<linear,7> lane<linear,8>
lane<linear,1,F> lane<linear,2,F> lane<linear,3,F> lane<linear,4,F> lane<linear,5,F> lane<linear,6,F> lane<linear,7,F> lane<linear,8,F>
lane<poly,1> lane<poly,2> lane<poly,3> lane<poly,4> lane<poly,5> lane<poly,6> lane<poly,7> lane<poly,8>
lane<poly,1,F> lane<poly,2,F> lane<poly,3,F> lane<poly,4,F> lane<poly,5,F> lane<poly,6,F> lane<poly,7,F> lane<poly,8,F>
lane<exp,2> lane<exp,4> lane<exp,6> lane<exp,8> lane<exp,2,F> lane<exp,4,F> lane<exp,6,F> lane<exp,8,F>
lane_phis<linear,1,2> lane_phis<linear,2,2> lane_phis<linear,3,2> lane_phis<linear,4,2> lane_phis<linear,5,2> lane_phis<linear,6,2>
lane_phis<linear,1,4> lane_phis<linear,2,4> lane_phis<linear,3,4> lane_phis<linear,4,4> lane_phis<linear,5,4> lane_phis<linear,6,4>
lane_phis<poly,1,2> lane_phis<poly,2,2> lane_phis<poly,3,2> lane_phis<poly,4,2> lane_phis<poly,5,2> lane_phis<poly,6,2>
lane_phis<poly,1,4> lane_phis<poly,2,4> lane_phis<poly,3,4> lane_phis<poly,4,4> lane_phis<poly,5,4> lane_phis<poly,6,4>
lane_phis<exp,2,2> lane_phis<exp,4,2> lane_phis<exp,6,2> lane_phis<exp,2,4> lane_phis<exp,4,4> lane_phis<exp,6,4>
lane_ar1<linear,1> lane_ar1<linear,2> lane_ar1<linear,3> lane_ar1<linear,4> lane_ar1<linear,5> lane_ar1<linear,6>
lane_ar1<linear,1,F> lane_ar1<linear,2,F> lane_ar1<linear,3,F> lane_ar1<linear,4,F> lane_ar1<linear,5,F> lane_ar1<linear,6,F>
lane_ar1<poly,1> lane_ar1<poly,2> lane_ar1<poly,3> lane_ar1<poly,4> lane_ar1<poly,1,F> lane_ar1<poly,2,F> lane_ar1<poly,3,F> lane_ar1<poly,4,F>
lane_ar1<exp,2> lane_ar1<exp,4> lane_ar1<exp,2,F> lane_ar1<exp,4,F>
lane_ar2<linear,2,2> lane_ar2<linear,2,3> lane_ar2<linear,2,4> lane_ar2<linear,2,2,F> lane_ar2<linear,2,3,F> lane_ar2<linear,2,4,F>
lane_ar2<linear,3,2> lane_ar2<linear,3,3> lane_ar2<linear,3,4> lane_ar2<linear,3,2,F> lane_ar2<linear,3,3,F> lane_ar2<linear,3,4,F>
lane_ar2<linear,4,2> lane_ar2<linear,4,3> lane_ar2<linear,4,4> lane_ar2<linear,4,2,F> lane_ar2<linear,4,3,F> lane_ar2<linear,4,4,F>
lane_ar2<poly,2,2> lane_ar2<poly,2,3> lane_ar2<poly,2,4> lane_ar2<poly,2,2,F> lane_ar2<poly,2,3,F> lane_ar2<poly,2,4,F>
lane_ar2<poly,3,2> lane_ar2<poly,3,3> lane_ar2<poly,3,4> lane_ar2<poly,3,2,F> lane_ar2<poly,3,3,F> lane_ar2<poly,3,4,F>
lane_ar2<exp,2,2> lane_ar2<exp,2,3> lane_ar2<exp,2,4> lane_ar2<exp,2,2,F> lane_ar2<exp,2,3,F> lane_ar2<exp,2,4,F>
lane_ar2<exp,4,2> lane_ar2<exp,4,3> lane_ar2<exp,4,4> lane_ar2<exp,4,2,F> lane_ar2<exp,4,3,F> lane_ar2<exp,4,4,F>
""".split()
# (see the module's docstring: no value to compare)
NOT_COMPARABLE = ["lane<poly,7>", "lane<poly,8>", "lane<poly,7,F>", "lane<poly,8,F>"]

# ---------------------------------------------------------------------------------------------
# The case tables. A case is (kernel, noise setting, options): the kernel's name WITHOUT its F suffix - kernel_for adds
# it - from which the model and the parameter count are read. Options: T (series length; default 25, 26 under two
# echoes, 40 for the exponential model), masked ("two": the third and the last timepoint, "last"), f64 (a float64
# series), conv (a convergence detector that watches F), V (voxels, default 197), gen (the voxel count the data are
# drawn for, of which the problem takes the first V), seed (added to the case's seed).
# The tests are parametrised over (case, need_f) pairs.
# ---------------------------------------------------------------------------------------------
WHITE = (["lane<linear,%d>" % p for p in range(1, 9)] + ["lane<poly,%d>" % p for p in range(1, 7)]
         + ["lane<exp,%d>" % p for p in (2, 4, 6, 8)])
PHIS_MODELS = [("linear", p) for p in range(1, 7)] + [("poly", p) for p in range(1, 7)] + [("exp", p) for p in (2, 4, 6)]
AR1_MODELS = [("linear", p) for p in range(1, 7)] + [("poly", p) for p in range(1, 5)] + [("exp", p) for p in (2, 4)]
AR2_MODELS = [("linear", 2), ("linear", 3), ("linear", 4), ("poly", 2), ("poly", 3), ("exp", 2), ("exp", 4)]


def both_ways(cases):
    return [(c, f) for c in cases for f in (False, True)]


# -- 1. every name once --
NAMES = both_ways(
    [(k, "white", {}) for k in WHITE]
    + [("lane_phis<%s,%d,2>" % mp, "12", {}) for mp in PHIS_MODELS]
    # (N = 4 with three and with four moment sets in use, alternating, so that every model meets both)
    + [("lane_phis<%s,%d,4>" % mp, "123" if i % 2 == 0 else "1234", {}) for i, mp in enumerate(PHIS_MODELS)]
    + [("lane_ar1<%s,%d>" % mp, "ar", {}) for mp in AR1_MODELS]
    + [("lane_ar2<%s,%d,%d>" % (mp + (na,)), "ar2" + cross, {}) for mp in AR2_MODELS for na, cross in ((2, "none"), (3, "same"), (4, "dual"))])

# -- 2. the other feeds and the watching instances --
# (a seed of its own for the masked cubic: with the case's ordinary draw the two CPU builds are 6.8e-7 apart on F, and
# test_cases_are_valid_for_the_oracle wants the draw to leave TOL_F / 3)
FEEDS = both_ways([(k, "white", dict(f64=True)) for k in WHITE]
                  + [(k, "white", dict(masked="two", seed=1) if k == "lane<poly,4>" else dict(masked="two")) for k in WHITE])
# (20 iterations per trial instead of five, so that the detector stops voxels and the saved state is taken back)
WATCH = dict(f64=True, conv="trialmode")
WATCHING = [(c, True) for c in [
    ("lane<linear,6>", "white", WATCH), ("lane<poly,4>", "white", WATCH), ("lane<exp,4>", "white", WATCH),
    ("lane_ar1<linear,5>", "ar", WATCH), ("lane_ar1<poly,2>", "ar", WATCH), ("lane_ar1<exp,2>", "ar", WATCH),
    ("lane_ar2<linear,3,3>", "ar2same", WATCH), ("lane_ar2<poly,2,4>", "ar2dual", WATCH), ("lane_ar2<exp,2,2>", "ar2none", WATCH)]]
PHIS_FEEDS = both_ways([
    ("lane_phis<linear,5,2>", "12", dict(f64=True)), ("lane_phis<poly,4,4>", "1234", dict(f64=True)), ("lane_phis<exp,4,2>", "12", dict(f64=True)),
    ("lane_phis<linear,4,4>", "123", dict(masked="last")), ("lane_phis<poly,2,2>", "12", dict(masked="last")),
    ("lane_phis<exp,2,4>", "1234", dict(masked="last"))])

# -- 3. series lengths, with F --
T_LIST = [7, 8, 9, 15, 16, 17, 23, 24, 33, 64, 65, 129, 130]
LENGTHS = [(c, True) for T in T_LIST for c in [
    ("lane<poly,3>", "white", dict(T=T)), ("lane<poly,3>", "white", dict(T=T, f64=True)), ("lane<poly,3>", "white", dict(T=T, masked="two")),
    ("lane<linear,5>", "white", dict(T=T)),       # above the SweepPark limit
    ("lane<exp,2>", "white", dict(T=T)),          # three waves per SIMD, the resynchronised exponentials
    ("lane_phis<poly,3,4>", "123", dict(T=T)),
    ("lane_ar1<linear,2>", "ar", dict(T=T))]]
# two echoes: the dispatcher takes lane_ar2 for an even number of timepoints from 8 on; an odd one is no valid
# configuration under two echoes at all, and 7 is the only length of the list below 8
LENGTHS += [(("lane_ar2<linear,2,4>", "ar2dual", dict(T=T)), True) for T in T_LIST if T % 2 == 0 and T >= 8]

# -- 4. the fallbacks behind a cancelled k'Qk, forced --
T_FORCED = [25, 70, 130]
FORCED = [(c, f) for T in T_FORCED for c, f in [
    # rescue_tiles (P <= 4: SweepPark::FITS)
    (("lane<exp,2>", "white", dict(T=T)), True), (("lane<exp,2>", "white", dict(T=T, f64=True)), True),
    (("lane<linear,4>", "white", dict(T=T)), True), (("lane<linear,4>", "white", dict(T=T, f64=True)), True),
    # rescue_residual in a tile-fed kernel
    (("lane<linear,5>", "white", dict(T=T)), False), (("lane<linear,8>", "white", dict(T=T)), True),
    # the series in place, with an incomplete last wavefront
    (("lane<poly,3>", "white", dict(T=T, masked="two")), True), (("lane<linear,6>", "white", dict(T=T, masked="two")), False),
    (("lane_phis<linear,3,2>", "12", dict(T=T)), False), (("lane_phis<exp,2,4>", "123", dict(T=T)), True),
    (("lane_ar1<linear,3>", "ar", dict(T=T)), True), (("lane_ar1<exp,2>", "ar", dict(T=T)), False)]]
# a single wavefront with 59 idle or repeating lanes
FORCED += [(("lane<linear,5>", "white", dict(T=70, V=5)), False)]

# -- 5. wavefront edges --
V_EDGES = [1, 63, 64, 65, V_EDGE_FULL]
EDGE_KINDS = [(("lane<poly,3>", "white", {}), True), (("lane<poly,3>", "white", dict(masked="two")), True),
              (("lane_ar1<linear,2>", "ar", {}), False), (("lane_phis<poly,3,2>", "12", {}), False)]
EDGES = [((k, n, dict(o, V=V, gen=V_EDGE_FULL)), f) for (k, n, o), f in EDGE_KINDS for V in V_EDGES]

ALL = NAMES + FEEDS + WATCHING + PHIS_FEEDS + LENGTHS + FORCED + EDGES

GEN_AMP = [1.0, 0.6, 0.4, 0.3]
GEN_RATE = [0.7, 6.0, 20.0, 50.0]
EXP_MEANS = np.log([x for pair in zip(GEN_AMP, GEN_RATE) for x in pair])  # amplitude, rate, amplitude, rate, ...


def parse_kernel(kernel):
    m = re.fullmatch(r"(lane|lane_phis|lane_ar1|lane_ar2)<(linear|poly|exp),(\d+)(?:,(\d))?>", kernel)
    assert m, kernel
    return m.group(1), m.group(2), int(m.group(3)), (int(m.group(4)) if m.group(4) else None)


def kernel_for(case, need_f):
    """the name hiplib.kernel_name answers: the kernels that evaluate F carry ',F' (the pattern kernels exist once)"""
    kernel = case[0]
    return kernel[:-1] + ",F>" if need_f and not kernel.startswith("lane_phis") else kernel


def case_id(pair):
    (kernel, noise, opt), need_f = pair
    return "-".join([kernel.replace("<", "_").rstrip(">"), noise]
                    + ["%s%s" % (k, "" if v is True else v) for k, v in sorted(opt.items())] + ["F" if need_f else "noF"])


def key_of(pair):
    (kernel, noise, opt), need_f = pair
    return kernel, noise, tuple(sorted(opt.items())), bool(need_f)


# ---------------------------------------------------------------------------------------------
# Problems
# ---------------------------------------------------------------------------------------------
def ar_noise(T, V, rho, sd, seed):
    rng = np.random.default_rng(seed)
    e = rng.normal(0, sd, (T, V))
    for t in range(1, T):
        e[t] += rho * e[t - 1]
    return e


def series_length(model, noise, opt):
    if "T" in opt:
        return opt["T"]
    return 40 if model == "exp" else (26 if noise.startswith("ar2") else 25)


def common_options(noise, opt, T, need_f):
    kw = dict(need_f=need_f, **NOISES[noise])
    if opt.get("masked"):
        kw["masked_timepoints"] = {"two": (3, T), "last": (T,)}[opt["masked"]]  # (1-based, as the reference's option)
    if opt.get("conv"):
        kw["convergence"] = opt["conv"]
    return kw


def as_series(y, opt):
    V = opt.get("V", V_DEFAULT)
    return np.ascontiguousarray(y[:, :V], dtype=np.float64 if opt.get("f64") else np.float32)


def linear_problem(case, need_f):
    """The linear and the polynomial entries: P regressors (the cosines cos(pi (t + 0.5) k / T), or the monomials of
    (t + 1) / T), coefficients N(0, 1) + 1, noise of standard deviation 0.2 (AR(1) with rho = 0.3 under the AR
    policies), five iterations."""
    kernel, noise, opt = case
    _, model, P, _ = parse_kernel(kernel)
    V, T = opt.get("V", V_DEFAULT), series_length(model, noise, opt)
    Vg = opt.get("gen", V)
    t = np.arange(T)
    X = np.cos(np.pi * (t[:, None] + 0.5) * np.arange(P)[None, :] / T) if model == "linear" else ((t[:, None] + 1.0) / T) ** np.arange(P)[None, :]
    seed = (1000 if model == "poly" else 0) + P + 37 * T + opt.get("seed", 0)
    coef = np.random.default_rng(100 + seed).normal(0, 1, (P, Vg)) + 1.0
    y = as_series(X @ coef + ar_noise(T, Vg, 0.3 if noise.startswith("ar") else 0.0, 0.2, 200 + seed), opt)
    kw = dict(max_iterations=20 if opt.get("conv") else 5, **common_options(noise, opt, T, need_f))
    if model == "poly":
        return vbabi.build_config(vbabi.MODEL_POLY, V, T, degree=P - 1, **kw), y
    return vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, **kw), y


def exp_problem(case, need_f):
    """The exponential entries: P / 2 exponentials of amplitudes 1, 0.6, 0.4, 0.3 and rates 0.7, 6, 20, 50 over
    t = 0 .. 2, a per-voxel amplitude scale U(0.8, 1.2), noise of standard deviation 0.02. One exponential (P = 2): the
    ordinary start, five iterations. More: started from its default posterior - equal rates - the fit is the chaotic one
    (DESIGN 5.2), so it starts from an image with separated rates instead, as tests/test_spatial_instantiations.py:
    the oracle's image after one iteration under the case's own noise settings (the right noise rows for every policy)
    with the model block of the covariance set to 0.05 I, no model-noise covariance, and the means at the values the
    data were generated from; three iterations from there."""
    kernel, noise, opt = case
    _, _, P, _ = parse_kernel(kernel)
    V, T = opt.get("V", V_DEFAULT), series_length("exp", noise, opt)
    Vg = opt.get("gen", V)
    dt = 2.0 / T
    t = np.arange(T) * dt
    clean = sum(a * np.exp(-r * t) for a, r in zip(GEN_AMP[:P // 2], GEN_RATE[:P // 2]))
    seed = 2000 + P + 37 * T + opt.get("seed", 0)
    scale = np.random.default_rng(100 + seed).uniform(0.8, 1.2, Vg)
    y = as_series(clean[:, None] * scale[None, :] + ar_noise(T, Vg, 0.3 if noise.startswith("ar") else 0.0, 0.02, 200 + seed), opt)
    kw = dict(num_exps=P // 2, dt=dt, **common_options(noise, opt, T, need_f))
    if P == 2:
        return vbabi.build_config(vbabi.MODEL_EXP, V, T, max_iterations=20 if opt.get("conv") else 5, **kw), y
    first = vbabi.build_config(vbabi.MODEL_EXP, V, T, max_iterations=1, **dict(kw, convergence="maxits"))
    img = oracle.run(first, y)["mvn"].copy()
    n = P + first.n_noise_outputs
    nCov = n * (n + 1) // 2
    for i in range(n):
        for j in range(min(i, P - 1) + 1):
            img[i * (i + 1) // 2 + j] = 0.05 if i == j else 0.0
    for i in range(P):
        img[nCov + i] = EXP_MEANS[i]
    return vbabi.build_config(vbabi.MODEL_EXP, V, T, max_iterations=3, init_mvn=img, **kw), y


def problem(pair):
    case, need_f = pair
    return exp_problem(case, need_f) if parse_kernel(case[0])[1] == "exp" else linear_problem(case, need_f)


def may_use_the_floor(case):
    """the exponential model (the floor includes the build with a 1-ulp exp) and the polynomial with six
    parameters (monomials up to t^5): DESIGN 5.2 lists them among the tests that opt in"""
    _, model, P, _ = parse_kernel(case[0])
    return model == "exp" or (model == "poly" and P == 6)


@functools.lru_cache(maxsize=None)
def _reference(key):
    kernel, noise, opt, need_f = key
    pair = ((kernel, noise, dict(opt)), need_f)
    h, y = problem(pair)
    cpu = [oracle.run(h, y), oracle.run_fma(h, y)]
    if h.cfg.model == vbabi.MODEL_EXP:
        # (the build whose exp has the device's accuracy class is one of the CPU builds - DESIGN 5.4)
        cpu.append(oracle.run_exp1ulp(h, y))
    for r in cpu:
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    y.setflags(write=False)
    return h, y, cpu


def reference(pair):
    """(holder, series, the CPU builds' results) of a case - computed once, shared by the tests that need it, left
    unchanged"""
    return _reference(key_of(pair))


# ---------------------------------------------------------------------------------------------
# CPU: the tables themselves, and the cases as problems for the oracle
# ---------------------------------------------------------------------------------------------
def test_every_compiled_name_has_a_case():
    """no entry of part 1 appears twice, every compiled name outside poly 7 / 8 appears, and every entry's name is of
    the family - with the N or NA - of the noise setting it is run with"""
    assert len(set(COMPILED)) == len(COMPILED) and set(NOT_COMPARABLE) < set(COMPILED)
    ids = [case_id(p) for p in NAMES]
    assert len(set(ids)) == len(ids)
    launched = [kernel_for(c, f) for c, f in NAMES]
    # (a pattern kernel exists once and runs with and without F: its name appears twice, every other name once)
    assert sorted(set(launched)) == sorted(set(COMPILED) - set(NOT_COMPARABLE))
    assert all(launched.count(k) == (2 if k.startswith("lane_phis") else 1) for k in launched)
    for (kernel, noise, opt), need_f in ALL:
        family, model, P, extra = parse_kernel(kernel)
        assert (family, extra) == FAMILY[noise], (kernel, noise)
        assert kernel_for((kernel, noise, opt), need_f) in COMPILED
        assert set(opt) <= {"T", "masked", "f64", "conv", "V", "gen", "seed"}, opt
        assert not (opt.get("masked") and noise.startswith("ar"))  # (the AR policies refuse masked timepoints)
        assert not opt.get("conv") or need_f
    for part in (NAMES, FEEDS, WATCHING, PHIS_FEEDS, LENGTHS, FORCED, EDGES):
        ids = [case_id(p) for p in part]
        assert len(set(ids)) == len(ids)
    # part 1: "three of four moment sets" and "all four" for every model
    for model in ("linear", "poly", "exp"):
        assert {n for (k, n, _), _ in NAMES if k.startswith("lane_phis<%s" % model) and k.endswith(",4>")} == {"123", "1234"}
    # part 2 derives from part 1's white-noise entries; part 3 holds every length for every kernel it names
    assert {c[0] for c, _ in FEEDS} == {c[0] for c, _ in NAMES if c[1] == "white"}
    assert {(c[0], c[2]["T"]) for c, _ in LENGTHS if c[1] != "ar2dual"} == {
        (k, T) for k in ("lane<poly,3>", "lane<linear,5>", "lane<exp,2>", "lane_phis<poly,3,4>", "lane_ar1<linear,2>") for T in T_LIST}
    assert [c[2]["T"] for c, _ in LENGTHS if c[1] == "ar2dual"] == [8, 16, 24, 64, 130]


def test_cases_are_valid_for_the_oracle():
    """(CPU) for every problem of every part: the oracle fails no voxel and every value is finite, all CPU builds take
    the same iteration counts, and - for every case that does not opt in to the floor - the two CPU builds agree within
    a third of the base tolerances on the means, the covariances and F. A condition on the inputs, not on the device:
    where a case misses it, its seed, length or pattern changes, never the bound."""
    seen = set()
    for pair in ALL:
        if key_of(pair) in seen:
            continue
        seen.add(key_of(pair))
        case, need_f = pair
        what = case_id(pair)
        h, y, cpu = reference(pair)
        assert h.cfg.n_voxels == case[2].get("V", V_DEFAULT) and bool(h.cfg.need_f) == need_f, what
        assert bool(h.cfg.data_f64) == bool(case[2].get("f64")), what
        for r in cpu:
            assert np.all(r["status"] == 0) and np.isfinite(r["mvn"]).all(), what
            assert np.array_equal(r["iterations"], cpu[0]["iterations"]), what
            if need_f:
                assert np.isfinite(r["free_energy"]).all(), what
        if may_use_the_floor(case):
            continue
        e_mean, e_cov, _ = parity.voxel_errors(h, cpu[0], cpu[1])
        assert e_mean.max() < parity.TOL_MEAN / 3 and e_cov.max() < parity.TOL_COV / 3, (what, e_mean.max(), e_cov.max())
        if need_f:
            Fa, Fb = cpu[0]["free_energy"], cpu[1]["free_energy"]
            e_f = np.max(np.abs(Fa - Fb) / np.maximum(1.0, np.abs(Fa)))
            assert e_f < parity.TOL_F / 3, (what, e_f)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def launch(pair, h, y):
    """the case on its lane kernel: the name first, so that a change of routing cannot turn the case into a test of
    another kernel"""
    hiplib.set_variant("lane")
    try:
        assert hiplib.kernel_name(h) == kernel_for(*pair), (hiplib.kernel_name(h), kernel_for(*pair))
        return hipengine.run(h, y)
    finally:
        hiplib.set_variant("auto")


def against_the_oracle(pair, got=None):
    case, need_f = pair
    h, y, cpu = reference(pair)
    if got is None:
        got = launch(pair, h, y)
    floor = may_use_the_floor(case)
    kw = dict(allow_floor=True) if floor else {}
    if case[2].get("conv"):
        # (a detector that watches F: a voxel whose change of F sits on the threshold may stop an iteration apart, as in
        # tests/test_random_configs.py)
        kw["allow_iter_mismatch"] = max(1, h.cfg.n_voxels // 50)
    r = parity.strict(h, cpu[0], got, what="lane " + case_id(pair), cpu2=cpu[1:], **kw)
    print("[lane instantiation] %s %s F=%d: means %.2e cov %.2e F %.2e%s"
          % (kernel_for(*pair), case_id(pair), need_f, r["err_means"], r["err_cov"], r["err_f"], " (raised)" if r["raised"] else ""))
    assert np.all(got["status"] == 0)
    assert floor or not r["raised"]
    return got


@gpu
@pytest.mark.parametrize("pair", NAMES, ids=case_id)
def test_every_name_against_the_oracle(pair):
    against_the_oracle(pair)


@gpu
@pytest.mark.parametrize("pair", FEEDS + PHIS_FEEDS, ids=case_id)
def test_the_other_feeds_against_the_oracle(pair):
    """float64: the fp64 tiles (lane_phis: the float64 series in place); masked timepoints: the series in place"""
    against_the_oracle(pair)


@gpu
@pytest.mark.parametrize("pair", WATCHING, ids=case_id)
def test_the_watching_instances_against_the_oracle(pair):
    """convergence=trialmode: the save buffer and the instance of the F kernels that watches F"""
    against_the_oracle(pair)


@gpu
@pytest.mark.parametrize("pair", LENGTHS, ids=case_id)
def test_series_lengths_against_the_oracle(pair):
    against_the_oracle(pair)


@gpu
@pytest.mark.parametrize("pair", FORCED, ids=case_id)
def test_forced_fallbacks_against_the_oracle_and_reversed(pair):
    """every voxel takes the direct sum in every iteration: strict parity with the oracle at the bounds of every other
    case, and the problem with its voxel order reversed returns the reversed result bit for bit"""
    h, y, _ = reference(pair)
    assert "init_mvn" not in h.keep  # (nothing per voxel but the series: reversing the series reverses the problem)
    hr, _ = problem(pair)
    hiplib.set_residual_tolerance(1.0)
    try:
        got = launch(pair, h, y)
        rev = launch(pair, hr, np.ascontiguousarray(y[:, ::-1]))
    finally:
        hiplib.set_residual_tolerance(1e-10)
    against_the_oracle(pair, got)
    for k in ("mvn", "free_energy", "status", "iterations"):
        assert np.array_equal(rev[k], got[k][..., ::-1], equal_nan=True), (case_id(pair), k)


_FULL_RUNS = {}


@gpu
@pytest.mark.parametrize("pair", EDGES, ids=case_id)
def test_wavefront_edges_against_the_oracle_and_the_full_run(pair):
    """1, 63, 64, 65 and 257 voxels: strict parity, and what a voxel gets is what it gets among 257"""
    (kernel, noise, opt), need_f = pair
    full_pair = ((kernel, noise, dict(opt, V=V_EDGE_FULL)), need_f)
    if key_of(full_pair) not in _FULL_RUNS:
        hf, yf, _ = reference(full_pair)
        _FULL_RUNS[key_of(full_pair)] = (launch(full_pair, hf, yf), yf)
    full, yf = _FULL_RUNS[key_of(full_pair)]
    h, y, _ = reference(pair)
    V = opt["V"]
    assert np.array_equal(y, yf[:, :V])
    got = against_the_oracle(pair)
    for k in ("mvn", "free_energy", "status", "iterations"):
        assert np.array_equal(got[k], full[k][..., :V], equal_nan=True), (case_id(pair), k)
