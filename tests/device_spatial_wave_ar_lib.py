"""Builds the test model library whose device bodies bring the wave-per-voxel spatial VB kernels under AR(1) noise
(tests/plugins/fwdmodel_spatial_wave_ar_models.hip: multiexp_spwa, linear_spwa, suppconv_spwa, multiexp_spwa_both) for the
tests and the measuring tool of those kernels, with device_model_lib's build of a library from its parts - and constructs
the problems those tests share: each one for the CPU oracle as a built-in model and for the library as its body, under
noise=ar with one echo and no cross terms, from the same initial posterior image. Nothing here needs a GPU."""
import numpy as np

import device_model_lib
from fabber_core_amd import hiplib, vbabi
from test_spatial import masked_volume
from test_spatial_wide import MIXED, cosine_design, smooth_linear_data

LIBRARY = "libfabber_models_spatial_wave_ar.so"
NAMES = ("multiexp_spwa", "linear_spwa", "suppconv_spwa", "multiexp_spwa_both")
AR = dict(noise=vbabi.NOISE_AR1, num_echoes=1)
SHAPE = (7, 6, 5)  # (the volume of tests/test_device_spatial_model.py)

# (P, T) of linear_spwa against the oracle, each for one way the lag-1 sums over chunks of 64 timepoints can go wrong: one
# partial chunk; exactly one chunk (the last row at the chunk's end, no hand-over); the lag pair (63, 64) across the
# boundary into a chunk of one timepoint; two hand-overs; the largest layout; a count served by this family because the
# name has no lane line
LINEAR_CASES = [(7, 21), (7, 64), (7, 65), (10, 129), (32, 70), (2, 21)]


def build_spatial_wave_ar_library():
    return device_model_lib.build("fwdmodel_spatial_wave_ar_models.hip", (1, 2, 3, 4, 5, 6), LIBRARY)


def volume():
    mask, coords = masked_volume(SHAPE, seed=61, keep=0.85)
    V = coords.shape[1]
    assert 128 < V < 192 and len(set(coords[2].tolist())) == 5
    return mask, coords


def ar_image(white, P, holder, alpha_post=None):
    """the initial posterior image as Vb::BuildInitialMvn writes it under AR(1) noise from the image under white noise
    (hiplib.initial_mvn): the model's block, then the alphas - N(0, 1e4 I) (noisemodel_ar.cc:379-403) or the (mean,
    covariance) of noise-initial-posterior - then the precision"""
    cfg = holder.cfg
    V = white.shape[1]
    nw, n = P + 1, P + 3
    assert white.shape[0] == vbabi.mvn_rows(nw)
    img = np.zeros((vbabi.mvn_rows(n), V))
    nCov = n * (n + 1) // 2
    for i in range(P):
        for j in range(i + 1):
            img[i * (i + 1) // 2 + j] = white[i * (i + 1) // 2 + j]
        img[nCov + i] = white[nw * (nw + 1) // 2 + i]
    mean, cov = alpha_post if alpha_post is not None else (np.zeros(2), 1e4 * np.eye(2))
    for a in range(2):
        q = P + a
        img[nCov + q] = mean[a]
        for a2 in range(a + 1):
            img[q * (q + 1) // 2 + P + a2] = cov[a][a2]
    b, c = cfg.noise_post_b[0], cfg.noise_post_c[0]
    q = P + 2
    img[q * (q + 1) // 2 + q] = b * b * c
    img[nCov + q] = b * c
    img[-1] = 1.0
    return img


def linear_problem(coords, P, T, need_f, iters=5, init_mvn=None, alpha_prior=None, alpha_post=None, seed=None):
    """(ref, dev, y): the design of P cosine regressors with the mixed priors of tests/test_spatial_wide.py (M, M, m, P, p,
    ARD, an image prior, then N; the first P of them) for the oracle as the built-in linear model and for the library as
    linear_spwa with the design in its constants block, both under noise=ar; the same initial posterior image with the
    means 1 / (k + 1) (away from zero: the reference's difference step is then 1e-5 of the mean and not its floor of
    1e-10)"""
    V = coords.shape[1]
    X = cosine_design(T, P)
    _, y = smooth_linear_data(coords, X, seed=P + 1 if seed is None else seed)
    ov = {"Parameter_%d" % (k + 1): dict(type=t) for k, t in enumerate(MIXED[:P])}
    images = {}
    k_img = MIXED.index("I")
    if k_img < P:
        ov["Parameter_%d" % (k_img + 1)] = dict(type="I", prec=4.0)
        images["Parameter_%d" % (k_img + 1)] = 0.2 + 0.05 * np.cos(coords[0] / 2.0)
    common = dict(max_iterations=iters, need_f=need_f, param_overrides=ov, image_priors=images)
    noise = dict(AR)
    if alpha_prior is not None:
        noise["ar_alpha_prior"] = alpha_prior
    if alpha_post is not None:
        noise["ar_alpha_post"] = alpha_post
    mvn = init_mvn
    if mvn is None:
        white = hiplib.initial_mvn(vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, **common), y)
        mvn = ar_image(white, P, vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, **common, **noise), alpha_post)
        n = P + 3
        for k in range(P):
            mvn[n * (n + 1) // 2 + k] = 1.0 / (k + 1)
    ref = vbabi.build_config(vbabi.MODEL_LINEAR, V, T, design=X, init_mvn=mvn, **common, **noise)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model="linear_spwa", constants=X,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_LINEAR, n_basis=P), init_mvn=mvn, **common, **noise)
    assert dev.cfg.n_phis == 1 == ref.cfg.n_phis and dev.cfg.noise == vbabi.NOISE_AR1
    return ref, dev, y


def planted_failures(y):
    """a NaN and an Inf sample in two voxels: (y with them, the voxels)"""
    y = np.array(y, copy=True)
    V = y.shape[1]
    bad = [V // 3, (2 * V) // 3]
    y[5, bad[0]] = np.nan
    y[17, bad[1]] = np.inf
    return y, bad


def exp_problem(coords, num, device_model="multiexp_spwa", T=60, **opts):
    """the construction of exp_problem in tests/test_device_spatial_wave_model.py (well-separated rates in the initial image,
    a prior M on amp1) under noise=ar"""
    V, dt = coords.shape[1], 0.01
    rates, amps = np.array([0.5, 3.0, 12.0, 40.0, 150.0])[:num], np.array([1.0, 0.8, 0.6, 0.4, 0.3])[:num]
    rng = np.random.default_rng(22)
    t = np.arange(T) * dt
    scale = 1.0 + 0.2 * np.sin(coords[0] / 2.0)
    y = sum(amps[i] * scale[None, :] * np.exp(-rates[i] * t)[:, None] for i in range(num)) + rng.normal(0, 0.02, (T, V))
    P = 2 * num
    white = hiplib.initial_mvn(vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=num, dt=dt), y)
    init = ar_image(white, P, vbabi.build_config(vbabi.MODEL_EXP, V, T, num_exps=num, dt=dt, **AR))
    n = P + 3
    nCov = n * (n + 1) // 2
    for i in range(num):
        init[nCov + 2 * i] = np.log(amps[i])
        init[nCov + 2 * i + 1] = np.log(rates[i])
    common = dict(num_exps=num, dt=dt, init_mvn=init, param_overrides={"amp1": dict(type="M")}, **AR, **opts)
    ref = vbabi.build_config(vbabi.MODEL_EXP, V, T, **common)
    dev = vbabi.build_config(vbabi.MODEL_PLUGIN, V, T, device_model=device_model,
                             params=vbabi.model_parameter_defaults(vbabi.MODEL_EXP, num_exps=num), **common)
    return ref, dev, y


def alpha_distributions():
    """an informative prior over the two AR coefficients with an off-diagonal precision, and an initial posterior with a
    covariance between them (test_ar_general.alpha_distributions): (mean, PRECISION matrix), (mean, COVARIANCE matrix)"""
    from test_ar_general import alpha_distributions as general
    return general(2, seed=42)


def oracle_cases(coords):
    """every problem the GPU tests hold to the oracle: name -> (ref, dev, y, exp1ulp, planted voxels)"""
    cases = {}
    for P, T in LINEAR_CASES:
        for need_f in (False, True):
            ref, dev, y = linear_problem(coords, P, T, need_f)
            cases["linear P=%d T=%d need_f=%d" % (P, T, need_f)] = (ref, dev, y, False, [])
    ref, dev, y = exp_problem(coords, 5, max_iterations=3)
    cases["five exponentials"] = (ref, dev, y, True, [])
    ref, dev, y = linear_problem(coords, 7, 21, True)
    y, bad = planted_failures(y)
    cases["failed voxels"] = (ref, dev, y, False, bad)
    prior, post = alpha_distributions()
    ref, dev, y = linear_problem(coords, 7, 21, True, alpha_prior=prior, alpha_post=post)
    cases["alphas from file"] = (ref, dev, y, False, [])
    ref, dev, y = exp_problem(coords, 2, max_iterations=3)
    cases["two exponentials"] = (ref, dev, y, True, [])
    return cases
