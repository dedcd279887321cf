/*
 * vb_api.hip - C ABI of the voxelwise VB engine (include/fabber_vb.h): validation, kernel
 * selection, launch, and the host-pointer convenience entry points.
 *
 * There is no CPU fallback: if no HIP device is present or a launch fails the call returns a
 * negative code and fabber_vb_last_error() says why.
 */
#include "vb_lane_launch.h"
#include "vb_host_stage.h"
#include "vb_device_registry.h"
#include "vb_wave_kernel.h"
#include "vb_postproc_kernel.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace fvb;

namespace fvb
{
// Device bodies that model libraries have registered (include/fabber_device_model.h), by name ...
template <> struct DeviceRegistryTraits<fvb_device_model>
{
    static constexpr const char *noun = "device model", *is = "is";
    static constexpr int first_code = -70;
    static std::vector<DeviceStructSize> sizes(const fvb_device_model &m)
    {
        return { { "KernelArgs", m.kernel_args_size, sizeof(KernelArgs) }, { "WaveLayout", m.wave_layout_size, sizeof(WaveLayout) } };
    }
    static const char *bad_params(const fvb_device_model &)
    {
        return nullptr;
    }
    static std::string entry(const std::string &name, int)
    {
        return "a device model named '" + name + "'";
    }
    static std::string absent(const std::string &name, int)
    {
        return "no device model '" + name + "' is registered";
    }
};
// ... and the lane-per-voxel kernels of such bodies (include/fabber_device_lane_model.h), by (name, parameter count):
// looked into only for a name the registry above holds.
template <> struct DeviceRegistryTraits<fvb_device_lane_model>
{
    static constexpr const char *noun = "device lane model", *is = "are";
    static constexpr int first_code = -70;
    static std::vector<DeviceStructSize> sizes(const fvb_device_lane_model &m)
    {
        return { { "KernelArgs", m.kernel_args_size, sizeof(KernelArgs) } };
    }
    static const char *bad_params(const fvb_device_lane_model &m)
    {
        return (m.n_params < 1 || m.n_params > 6 || m.save_rows < 0) ? "the lane kernels of a library body exist for 1 to 6" : nullptr;
    }
    static std::string entry(const std::string &name, int n_params)
    {
        return "lane kernels of a device model named '" + name + "' with " + std::to_string(n_params) + " parameters";
    }
    static std::string absent(const std::string &name, int n_params)
    {
        return "no lane kernels of a device model '" + name + "' with " + std::to_string(n_params) + " parameters are registered";
    }
};
// ... and their lane-per-voxel kernels under AR(1) noise and noise patterns (include/fabber_device_lane_noise_model.h), by
// (name, parameter count): a registry of its own, an entry says which of the two families its library compiled.
template <> struct DeviceRegistryTraits<fvb_device_lane_noise_model>
{
    static constexpr const char *noun = "device lane noise model", *is = "are";
    static constexpr int first_code = -70;
    static std::vector<DeviceStructSize> sizes(const fvb_device_lane_noise_model &m)
    {
        return { { "KernelArgs", m.kernel_args_size, sizeof(KernelArgs) } };
    }
    static const char *bad_params(const fvb_device_lane_noise_model &m)
    {
        if (m.n_params < 1 || m.n_params > 6)
            return "the lane kernels of a library body exist for 1 to 6";
        if (m.families == 0 || (m.families & ~(FVB_LANE_NOISE_AR1 | FVB_LANE_NOISE_PHIS)) != 0)
            return "the families mask names none of FVB_LANE_NOISE_AR1 and FVB_LANE_NOISE_PHIS, or a family this engine does not know";
        return (m.save_rows_ar1 < 0 || m.save_rows_phis2 < 0 || m.save_rows_phis4 < 0) ? "a negative row count of the save buffer" : nullptr;
    }
    static std::string entry(const std::string &name, int n_params)
    {
        return "AR(1) / noise-pattern lane kernels of a device model named '" + name + "' with " + std::to_string(n_params) + " parameters";
    }
    static std::string absent(const std::string &name, int n_params)
    {
        return "no AR(1) / noise-pattern lane kernels of a device model '" + name + "' with " + std::to_string(n_params)
            + " parameters are registered";
    }
};
// ... and the result-image kernel of such bodies (include/fabber_device_results_model.h), by name: the kernel takes any
// parameter count. Looked into only for a name the first registry holds.
template <> struct DeviceRegistryTraits<fvb_device_results_model>
{
    static constexpr const char *noun = "device results model", *is = "is";
    static constexpr int first_code = -80;
    static std::vector<DeviceStructSize> sizes(const fvb_device_results_model &m)
    {
        return { { "fvb_config", m.config_size, sizeof(fvb_config) }, { "fvb_postproc", m.postproc_size, sizeof(fvb_postproc) } };
    }
    static const char *bad_params(const fvb_device_results_model &)
    {
        return nullptr;
    }
    static std::string entry(const std::string &name, int)
    {
        return "the result-image kernel of a device model named '" + name + "'";
    }
    static std::string absent(const std::string &name, int)
    {
        return "no result-image kernel of a device model '" + name + "' is registered";
    }
};
// ... and their initial-posterior kernel (include/fabber_device_init_model.h), by name: any parameter count. Looked into
// only for a name the first registry holds.
template <> struct DeviceRegistryTraits<fvb_device_init_model>
{
    static constexpr const char *noun = "device init model", *is = "is";
    static constexpr int first_code = -90;
    static std::vector<DeviceStructSize> sizes(const fvb_device_init_model &m)
    {
        return { { "fvb_config", m.config_size, sizeof(fvb_config) } };
    }
    static const char *bad_params(const fvb_device_init_model &)
    {
        return nullptr;
    }
    static std::string entry(const std::string &name, int)
    {
        return "the initial-posterior kernel of a device model named '" + name + "'";
    }
    static std::string absent(const std::string &name, int)
    {
        return "no initial-posterior kernel of a device model '" + name + "' is registered";
    }
};
} // namespace fvb

namespace
{
thread_local std::string g_last_error;
int g_variant = 0; // 0 auto, 1 lane, 2 wave
int g_residual_mode = 0; // 0 adaptive, 1 always exact, 2 moments only
// linearisations of a run that evaluate the model pointwise (vb_lane_kernel.h); the environment variable is an experiment switch
int g_precise_passes = getenv("FVB_PRECISE_PASSES") ? atoi(getenv("FVB_PRECISE_PASSES")) : -1; // -1: by model, see run_device_as
bool g_tiled = getenv("FVB_NO_TILES") == nullptr; // experiment switch: FVB_NO_TILES=1 keeps the in-place (strided) feed
double g_residual_tol = 1e-10; // moments value keeps >= 6 significant digits where it is used

int fail(int code, const std::string &msg)
{
    g_last_error = msg;
    return code;
}

thread_local std::string g_kernel_name; // fabber_vb_kernel_name of a registered body: "wave<NAME>", "lane<NAME,P>", "lane_ar1<NAME,P>", ...

int validate(const fvb_config *cfg, bool allow_spatial = false, bool allow_no_noise = false)
{
    if (!cfg)
        return fail(-1, "config is NULL");
    if (cfg->abi_version != FVB_ABI_VERSION)
        return fail(-2, "fvb_config.abi_version mismatch");
    if (cfg->n_voxels < 0 || cfg->n_times <= 0)
        return fail(-3, "bad n_voxels / n_times");
    if (cfg->n_params <= 0 || cfg->n_params > (cfg->params_ext ? FVB_MAX_PARAMS_EXT : FVB_MAX_PARAMS))
        return fail(-4, cfg->params_ext ? "n_params out of range" : "n_params out of range (more than FVB_MAX_PARAMS parameters: fvb_config.params_ext)");
    // (allow_no_noise: the post-processing of a result image, which such problems have like any other)
    if (cfg->params_ext && allow_spatial && !allow_no_noise)
        return fail(-4, "a parameter table (more than FVB_MAX_PARAMS parameters) runs voxelwise VB and method=nlls only");
    // (a result image without noise entries - method=nlls - can only be post-processed)
    if ((cfg->n_phis <= 0 && !(allow_no_noise && cfg->n_phis == 0)) || cfg->n_phis > FVB_MAX_PHIS)
        return fail(-5, "n_phis out of range");
    if (cfg->noise != FVB_NOISE_WHITE && cfg->noise != FVB_NOISE_AR1)
        return fail(-6, "noise model not supported by this build");
    if (cfg->noise == FVB_NOISE_AR1) // noisemodel_ar.cc:322-349
    {
        if (cfg->n_phis != 1 && cfg->n_phis != 2)
            return fail(-6, "AR(1) noise: num-echoes must be 1 or 2");
        if (cfg->ar_cross_terms < 0 || cfg->ar_cross_terms > 2)
            return fail(-6, "AR(1) noise: unknown ar1-cross-terms");
        if (cfg->n_phis == 1 && cfg->ar_cross_terms != 0)
            return fail(-6, "AR(1) noise: you must use ar1-cross-terms=none with num-echoes=1");
        if (cfg->n_times % cfg->n_phis != 0)
            return fail(-6, "AR(1) noise: the number of timepoints is not a multiple of num-echoes");
    }
    if (cfg->convergence < FVB_CONV_MAXITS || cfg->convergence > FVB_CONV_LM)
        return fail(-7, "unknown convergence detector");
    if (cfg->max_iterations <= 0)
        return fail(-8, "max_iterations must be positive");
    if (cfg->convergence != FVB_CONV_MAXITS && !cfg->need_f)
        return fail(-9, "convergence detector uses F but need_f is 0");
    if (cfg->model == FVB_MODEL_LINEAR && !cfg->design)
        return fail(-10, "linear model needs a design matrix");
    if (cfg->model == FVB_MODEL_EXP && (cfg->n_params != 2 * cfg->model_iopt[0]))
        return fail(-11, "exp model: n_params != 2 * num-exps");
    if (cfg->model == FVB_MODEL_POLY && (cfg->n_params != cfg->model_iopt[0] + 1))
        return fail(-12, "poly model: n_params != degree + 1");
    if (cfg->model == FVB_MODEL_PLUGIN)
        if (int rc = check_device_model_config(cfg))
            return rc;
    for (int k = 0; k < cfg->n_params; k++)
    {
        // (validate() sees the configuration as the caller built it: with device entry points the table itself is device
        // memory and is not looked into here)
        if (cfg->params_ext)
            break;
        if (cfg->prior_type[k] == FVB_PRIOR_IMAGE && !cfg->image_prior[k])
            return fail(-13, "image prior without an image");
        if (cfg->prior_type[k] > FVB_PRIOR_ARD && !allow_spatial)
            return fail(-14, "spatial priors are not handled by the voxelwise engine (use fabber_vb_run_spatial_*)");
        if (cfg->prior_type[k] < 0 || cfg->prior_type[k] > FVB_PRIOR_SPATIAL_p)
            return fail(-14, "unknown prior type");
    }
    return 0;
}

// Below this many voxels the lane kernel (V/64 wavefronts, each taking the full per-voxel latency)
// leaves most of the 1024 SIMDs empty and the wave-per-voxel kernel (V wavefronts) finishes
// first. Measured crossovers on MI355X (profiles/r1_lane_vs_wave.jsonl): ~6k voxels for the
// bi-exponential C3 fit (lane 2.2 ms flat, wave 0.4 us per voxel), ~2.5k for the single-exponential
// C2 fit (lane 0.12 ms flat, wave 0.04 us per voxel).
constexpr int WAVE_KERNEL_BELOW_VOXELS = 4096;

// The lane kernels a configuration runs on: the engine's own (k) or, for a body from a model library, the ones its
// library compiled (launch: the library's launcher, white noise with one precision; noise_launch: the one of its AR(1) and
// noise-pattern kernels, with the family and, for a pattern, the moment sets N of the kernel; of k only save_rows is
// set). Neither: the wave-per-voxel kernels.
struct LaneRoute
{
    LaneKernelInfo k{ nullptr, 0, nullptr };
    fvb_device_lane_launch_fn launch = nullptr;
    fvb_device_lane_noise_launch_fn noise_launch = nullptr;
    int family = 0, pattern_n = 0;
    // the feeds the route has kernels for: the caller's image in place, the tiled series
    bool has_strided = false, has_tiles = false;
    bool any() const
    {
        return has_strided || has_tiles;
    }
    bool library() const
    {
        return launch || noise_launch;
    }
};

// the size rule of the white-noise lane kernels: false = the wave-per-voxel kernel finishes first
bool lane_worth_it(const fvb_config *cfg, double evaluations)
{
    // ... for models whose re-linearisation is long enough to be worth sharing out over 64 lanes: T (2P + 1) model
    // evaluations per pass, an exponential counted twice. Below ~400 of them (C1: a quadratic over 10 timepoints = 70)
    // the wave kernel's per-iteration synchronisation outweighs what it shares, whatever the voxel count: 512 voxels
    // of C1 take 0.058 ms on the lane kernel against 0.105 ms.
    return !(g_variant == 0 && cfg->noise == FVB_NOISE_WHITE && cfg->n_voxels < WAVE_KERNEL_BELOW_VOXELS && evaluations >= 400
        && wave_layout(cfg->n_times, cfg->n_params, cfg->n_phis).bytes <= 160 * 1024);
}

LaneKernelInfo select_builtin_lane(const fvb_config *cfg)
{
    if (g_variant == 2 || (cfg->n_phis != 1 && cfg->noise == FVB_NOISE_WHITE && cfg->n_phis > 4))
        return LaneKernelInfo{ nullptr, 0, nullptr };
    if (cfg->noise == FVB_NOISE_AR1 && cfg->n_phis == 2) // two echoes: the two-pass kernel of vb_lane_arn_kernel.h
    {
        if (cfg->n_times % 2 != 0 || cfg->n_times < 8 || (g_variant == 0 && cfg->n_voxels < WAVE_KERNEL_BELOW_VOXELS))
            return LaneKernelInfo{ nullptr, 0, nullptr };
        const int n_alphas = 2 + cfg->ar_cross_terms;
        const bool f = cfg->need_f != 0;
        switch (cfg->model)
        {
        case FVB_MODEL_POLY:
            return get_lane_arn_kernel_poly(cfg->n_params, n_alphas, f);
        case FVB_MODEL_LINEAR:
            return get_lane_arn_kernel_linear(cfg->n_params, n_alphas, f);
        case FVB_MODEL_EXP:
            return get_lane_arn_kernel_exp(cfg->n_params, n_alphas, f);
        default:
            return LaneKernelInfo{ nullptr, 0, nullptr };
        }
    }
    if (cfg->n_phis != 1 && cfg->noise != FVB_NOISE_WHITE)
        return LaneKernelInfo{ nullptr, 0, nullptr };
    const double evaluations = (double)cfg->n_times * (2 * cfg->n_params + 1) * (cfg->model == FVB_MODEL_EXP ? 2.0 : 1.0);
    if (!lane_worth_it(cfg, evaluations))
        return LaneKernelInfo{ nullptr, 0, nullptr };
    const bool need_f = cfg->need_f != 0;
    if (cfg->noise == FVB_NOISE_WHITE && cfg->n_phis > 1) // noise-pattern: 2 .. 4 precisions
    {
        if (cfg->n_times > 32768) // (the kernel keeps the class of every timepoint in LDS, one byte each)
            return LaneKernelInfo{ nullptr, 0, nullptr };
        const bool two = cfg->n_phis == 2;
        switch (cfg->model)
        {
        case FVB_MODEL_POLY:
            return two ? get_lane_pattern_kernel_poly_2(cfg->n_params) : get_lane_pattern_kernel_poly_4(cfg->n_params);
        case FVB_MODEL_LINEAR:
            return two ? get_lane_pattern_kernel_linear_2(cfg->n_params) : get_lane_pattern_kernel_linear_4(cfg->n_params);
        case FVB_MODEL_EXP:
            return two ? get_lane_pattern_kernel_exp_2(cfg->n_params) : get_lane_pattern_kernel_exp_4(cfg->n_params);
        default:
            return LaneKernelInfo{ nullptr, 0, nullptr };
        }
    }
    if (cfg->noise == FVB_NOISE_AR1)
    {
        switch (cfg->model)
        {
        case FVB_MODEL_POLY:
            return get_lane_ar_kernel_poly(cfg->n_params, need_f);
        case FVB_MODEL_LINEAR:
            return get_lane_ar_kernel_linear(cfg->n_params, need_f);
        case FVB_MODEL_EXP:
            return get_lane_ar_kernel_exp(cfg->n_params, need_f);
        default:
            return LaneKernelInfo{ nullptr, 0, nullptr };
        }
    }
    switch (cfg->model)
    {
    case FVB_MODEL_POLY:
        return get_lane_kernel_poly(cfg->n_params, need_f);
    case FVB_MODEL_LINEAR:
        return get_lane_kernel_linear(cfg->n_params, need_f);
    case FVB_MODEL_EXP:
        return get_lane_kernel_exp(cfg->n_params, need_f);
    default:
        return LaneKernelInfo{ nullptr, 0, nullptr };
    }
}

LaneRoute select_lane(const fvb_config *cfg)
{
    LaneRoute route;
    if (cfg->model != FVB_MODEL_PLUGIN)
    {
        route.k = select_builtin_lane(cfg);
        route.has_strided = route.k.fn != nullptr;
        route.has_tiles = route.k.fn_tiles_f32 != nullptr;
        return route;
    }
    // A body from a model library: its lane kernels exist for the parameter counts and the noise models its library
    // registered; the wave-per-voxel kernels of the body take everything else (a body's evaluation is counted once in
    // the size rule).
    if (g_variant == 2)
        return route;
    const double evaluations = (double)cfg->n_times * (2 * cfg->n_params + 1);
    if (cfg->noise == FVB_NOISE_WHITE && cfg->n_phis == 1) // include/fabber_device_lane_model.h: all three feeds
    {
        fvb_device_lane_model entry;
        if (lane_worth_it(cfg, evaluations) && DeviceRegistry<fvb_device_lane_model>::instance().find(config_device_model(cfg), cfg->n_params, &entry))
        {
            route.launch = entry.launch;
            route.k.save_rows = entry.save_rows;
            route.has_strided = route.has_tiles = true;
        }
        return route;
    }
    // include/fabber_device_lane_noise_model.h, under the conditions select_builtin_lane places on the built-in kernels
    // of the family: AR(1) with one echo (no size rule, tiles only), 2 to 4 precisions (the class bytes fit LDS, the
    // size rule; the series in place only). Two echoes and 5 to 8 precisions: the wave kernels.
    const bool ar1 = cfg->noise == FVB_NOISE_AR1 && cfg->n_phis == 1;
    const bool phis = cfg->noise == FVB_NOISE_WHITE && cfg->n_phis >= 2 && cfg->n_phis <= 4;
    if (!ar1 && !(phis && cfg->n_times <= 32768 && lane_worth_it(cfg, evaluations)))
        return route;
    fvb_device_lane_noise_model entry;
    const int family = ar1 ? FVB_LANE_NOISE_AR1 : FVB_LANE_NOISE_PHIS;
    if (DeviceRegistry<fvb_device_lane_noise_model>::instance().find(config_device_model(cfg), cfg->n_params, &entry)
        && (entry.families & family) != 0)
    {
        route.noise_launch = entry.launch;
        route.family = family;
        route.pattern_n = ar1 ? 0 : (cfg->n_phis == 2 ? 2 : 4);
        route.k.save_rows = ar1 ? entry.save_rows_ar1 : (route.pattern_n == 2 ? entry.save_rows_phis2 : entry.save_rows_phis4);
        route.has_tiles = ar1;
        route.has_strided = !ar1;
    }
    return route;
}

// Where the model fit and the residuals of a (validated) configuration come from: the engine's kernel for its own
// models; for a body of a model library the kernel its library compiled around it (include/fabber_device_results_model.h)
// - an entry counts next to a wave body of its name - and without one nothing: the engine has no evaluator for the body.
struct PostprocRoute
{
    bool fit = false;                               // a model fit can be computed
    fvb_device_results_launch_fn library = nullptr; // ... by this launcher (NULL: by the engine's kernel)
    std::string name;                               // fabber_vb_postproc_kernel_name
};

PostprocRoute select_postproc(const fvb_config *cfg)
{
    PostprocRoute route;
    if (cfg->model != FVB_MODEL_PLUGIN)
    {
        route.fit = true;
        route.name = "postproc";
        return route;
    }
    const std::string model = config_device_model(cfg);
    fvb_device_results_model entry;
    if (find_wave_body(model) && DeviceRegistry<fvb_device_results_model>::instance().find(model, 0, &entry))
    {
        route.fit = true;
        route.library = entry.launch;
        route.name = "postproc<" + model + ">";
    }
    return route;
}

thread_local std::string g_postproc_kernel_name;

bool needs_save(const fvb_config *cfg)
{
    return cfg->convergence == FVB_CONV_FREDUCE || cfg->convergence == FVB_CONV_TRIALMODE
        || cfg->convergence == FVB_CONV_LM;
}

} // namespace

// helpers shared with vb_spatial_api.hip
namespace fvb
{
int api_fail(int code, const std::string &msg)
{
    return fail(code, msg);
}
int api_validate(const fvb_config *cfg, bool allow_spatial)
{
    return validate(cfg, allow_spatial);
}
int api_variant()
{
    return g_variant;
}
int api_residual_mode()
{
    return g_residual_mode;
}
int api_precise_passes()
{
    return g_precise_passes >= 0 ? g_precise_passes : 2; // (see run_device_as)
}
double api_residual_tol()
{
    return g_residual_tol;
}
// Work buffers of the size of the series are allocated by every run; they come from a stream-ordered memory pool
// that keeps freed memory instead of returning it to the driver at the next synchronisation. The pool is the
// LIBRARY'S OWN (one per device, created on first use): the process-wide default pool of an embedding application
// keeps its settings. fabber_vb_release_cached_memory gives everything back, on every device that was used.
struct PoolTable
{
    std::mutex lock;
    std::vector<std::pair<int, hipMemPool_t> > pools; // (device, pool); pool == nullptr: the default pool is used
};
static PoolTable &pool_table()
{
    static PoolTable t;
    return t;
}
// the current device's pool (nullptr: creation is not supported here - plain hipMallocAsync from the default pool)
hipMemPool_t api_pool()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        return nullptr;
    PoolTable &t = pool_table();
    std::lock_guard<std::mutex> hold(t.lock);
    for (auto &e : t.pools)
        if (e.first == dev)
            return e.second;
    hipMemPool_t pool = nullptr;
    hipMemPoolProps props;
    memset(&props, 0, sizeof(props));
    props.allocType = hipMemAllocationTypePinned;
    props.handleTypes = hipMemHandleTypeNone;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = dev;
    if (hipMemPoolCreate(&pool, &props) == hipSuccess)
    {
        uint64_t never = UINT64_MAX;
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &never);
    }
    else
    {
        (void)hipGetLastError();
        pool = nullptr;
    }
    t.pools.push_back(std::make_pair(dev, pool));
    return pool;
}
hipError_t api_pool_free(void *p, hipStream_t stream)
{
    return hipFreeAsync(p, stream);
}
hipError_t api_pool_alloc(void **p, size_t bytes, hipStream_t stream)
{
    hipMemPool_t pool = api_pool();
    const hipError_t e = pool ? hipMallocFromPoolAsync(p, bytes, pool, stream) : hipMallocAsync(p, bytes, stream);
    if (e != hipSuccess)
        return e;
    // The allocation is waited for: what follows is often a copy from pageable host memory, which the runtime carries out
    // outside the stream's order - and under ROCm 7.2's runtime such a copy into memory the pool had only just mapped
    // arrived incomplete (tools/measure/runtime_check_release.py: wrong results from the first run after the pools had
    // been given back). The callers allocate at the start of a run, when the stream has nothing pending.
    return hipStreamSynchronize(stream);
}
void api_keep_pool_memory()
{
    (void)api_pool();
}
// A non-blocking stream beside the caller's (the spatial run's set-up kernel runs on one while the geometry is worked out):
// kept between runs, because creating and destroying a stream costs 0.5 - 1.2 ms each (tools/measure/host_timeline.sh) -
// of a 20 ms spatial run. Per device; fabber_vb_release_cached_memory destroys the idle ones.
struct SideStreams
{
    std::mutex lock;
    std::vector<std::pair<int, hipStream_t> > idle;
};
static SideStreams &side_streams()
{
    static SideStreams s;
    return s;
}
hipError_t api_take_side_stream(hipStream_t *out, int *device)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return e;
    *device = dev;
    {
        SideStreams &c = side_streams();
        std::lock_guard<std::mutex> hold(c.lock);
        for (size_t i = 0; i < c.idle.size(); i++)
            if (c.idle[i].first == dev)
            {
                *out = c.idle[i].second;
                c.idle.erase(c.idle.begin() + (long)i);
                return hipSuccess;
            }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
// (the stream must be idle: the caller has synchronised it)
void api_return_side_stream(hipStream_t s, int dev)
{
    SideStreams &c = side_streams();
    std::lock_guard<std::mutex> hold(c.lock);
    c.idle.push_back(std::make_pair(dev, s));
}
void destroy_side_streams()
{
    SideStreams &c = side_streams();
    std::lock_guard<std::mutex> hold(c.lock);
    int now = 0;
    (void)hipGetDevice(&now);
    for (auto &e : c.idle)
        if (hipSetDevice(e.first) == hipSuccess)
            (void)hipStreamDestroy(e.second);
    c.idle.clear();
    (void)hipSetDevice(now);
}

// keep_bytes: what every pool may keep for the next run (0 = give everything back). A pool that holds more is DESTROYED
// (the next allocation makes a new one) rather than trimmed: under ROCm 7.2's runtime the first run after
// hipMemPoolTrimTo(pool, 0) came back with wrong results - every voxel of a one-stream, one-block call
// (tools/measure/runtime_check_release.py; ROCm 7.0's runtime did not show it) - and a destroyed pool has no such state.
void api_release_pools(uint64_t keep_bytes)
{
    PoolTable &t = pool_table();
    std::lock_guard<std::mutex> hold(t.lock);
    int before = 0;
    (void)hipGetDevice(&before);
    for (size_t i = 0; i < t.pools.size();)
    {
        auto &e = t.pools[i];
        if (hipSetDevice(e.first) != hipSuccess)
        {
            i++;
            continue;
        }
        hipMemPool_t pool = e.second;
        const bool own = pool != nullptr;
        if (!own && hipDeviceGetDefaultMemPool(&pool, e.first) != hipSuccess)
        {
            i++;
            continue;
        }
        // (nothing to give back: no need to wait for the device - fabber_destroy calls this when the last handle goes)
        uint64_t reserved = UINT64_MAX;
        if (hipMemPoolGetAttribute(pool, hipMemPoolAttrReservedMemCurrent, &reserved) == hipSuccess && reserved <= keep_bytes)
        {
            i++;
            continue;
        }
        (void)hipGetLastError();
        (void)hipDeviceSynchronize();
        if (own)
        {
            (void)hipMemPoolDestroy(pool);
            t.pools.erase(t.pools.begin() + (long)i); // (api_pool() creates the next one)
            continue;
        }
        (void)hipMemPoolTrimTo(pool, (size_t)keep_bytes); // (the device's default pool, where no pool of our own could be made)
        i++;
    }
    (void)hipSetDevice(before);
}
} // namespace fvb

__global__ __launch_bounds__(64) void device_math_kernel(int what, int n, const double *in, double *out)
{
    __shared__ double exp_tab[64];
    exp_tab[threadIdx.x] = FVB_EXP_TABLE[threadIdx.x]; // (as the kernels that use exp_acc do: vb_spatial.h)
    __syncthreads();
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n)
        return;
    if (what == 0)
        out[i] = exp_acc(in[i], exp_tab);
    else if (what == 1)
        out[i] = exp(in[i]);
    else
    {
        double a[10], r[10], logabs;
        int sign;
        for (int k = 0; k < 10; k++)
            a[k] = in[(size_t)i * 10 + k];
        const bool ok = mvn_invert<4>(a, r, logabs, sign);
        for (int k = 0; k < 10; k++)
            out[(size_t)i * 11 + k] = ok ? r[k] : __builtin_nan("");
        out[(size_t)i * 11 + 10] = logabs;
    }
}

namespace
{
void destroy_idle_pipe_streams();
}

extern "C" {

int32_t fabber_vb_mvn_rows(int32_t n)
{
    return n * (n + 1) / 2 + n + 1;
}

int32_t fabber_vb_abi_version(void)
{
    return FVB_ABI_VERSION;
}

int32_t fabber_vb_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

const char *fabber_vb_last_error(void)
{
    return g_last_error.c_str();
}

void fabber_vb_release_cached_memory(void)
{
    destroy_idle_pipe_streams();
    fvb::destroy_side_streams();
    fvb::api_release_pools(0);
}

void fabber_vb_trim_cached_memory(uint64_t keep_bytes)
{
    fvb::api_release_pools(keep_bytes);
}

int32_t fabber_vb_pin_host_buffer(void *ptr, uint64_t bytes)
{
    if (!ptr || bytes == 0)
        return fail(-23, "fabber_vb_pin_host_buffer: NULL pointer or empty range");
    FVB_HIP_CHECK(hipHostRegister(ptr, (size_t)bytes, hipHostRegisterPortable));
    return 0;
}

int32_t fabber_vb_unpin_host_buffer(void *ptr)
{
    if (!ptr)
        return fail(-23, "fabber_vb_unpin_host_buffer: NULL pointer");
    FVB_HIP_CHECK(hipHostUnregister(ptr));
    return 0;
}

void fabber_vb_set_variant(int32_t variant)
{
    g_variant = variant;
}

void fabber_vb_set_residual_mode(int32_t mode)
{
    g_residual_mode = mode;
}

void fabber_vb_set_residual_tolerance(double tol)
{
    g_residual_tol = tol;
}

int32_t fabber_vb_register_device_model(const fvb_device_model *model)
{
    return DeviceRegistry<fvb_device_model>::instance().add(model);
}

int32_t fabber_vb_unregister_device_model(const char *name)
{
    return DeviceRegistry<fvb_device_model>::instance().remove(name, 0);
}

int32_t fabber_vb_device_model_count(void)
{
    return DeviceRegistry<fvb_device_model>::instance().count();
}

const char *fabber_vb_device_model_name(int32_t i)
{
    return DeviceRegistry<fvb_device_model>::instance().name(i);
}

int32_t fabber_vb_register_device_lane_model(const fvb_device_lane_model *model)
{
    return DeviceRegistry<fvb_device_lane_model>::instance().add(model);
}

int32_t fabber_vb_unregister_device_lane_model(const char *name, int32_t n_params)
{
    return DeviceRegistry<fvb_device_lane_model>::instance().remove(name, n_params);
}

int32_t fabber_vb_device_lane_model_count(void)
{
    return DeviceRegistry<fvb_device_lane_model>::instance().count();
}

const char *fabber_vb_device_lane_model_name(int32_t i)
{
    return DeviceRegistry<fvb_device_lane_model>::instance().name(i);
}

int32_t fabber_vb_device_lane_model_params(int32_t i)
{
    return DeviceRegistry<fvb_device_lane_model>::instance().params(i, 0);
}

int32_t fabber_vb_register_device_lane_noise_model(const fvb_device_lane_noise_model *model)
{
    return DeviceRegistry<fvb_device_lane_noise_model>::instance().add(model);
}

int32_t fabber_vb_unregister_device_lane_noise_model(const char *name, int32_t n_params)
{
    return DeviceRegistry<fvb_device_lane_noise_model>::instance().remove(name, n_params);
}

int32_t fabber_vb_device_lane_noise_model_count(void)
{
    return DeviceRegistry<fvb_device_lane_noise_model>::instance().count();
}

const char *fabber_vb_device_lane_noise_model_name(int32_t i)
{
    return DeviceRegistry<fvb_device_lane_noise_model>::instance().name(i);
}

int32_t fabber_vb_device_lane_noise_model_params(int32_t i)
{
    return DeviceRegistry<fvb_device_lane_noise_model>::instance().params(i, 0);
}

int32_t fabber_vb_find_device_lane_noise_model(const char *name, int32_t n_params, fvb_device_lane_noise_model *entry)
{
    return (name && entry && DeviceRegistry<fvb_device_lane_noise_model>::instance().find(name, n_params, entry)) ? 1 : 0;
}

const char *fabber_vb_kernel_name(const fvb_config *cfg)
{
    if (validate(cfg) != 0)
        return "invalid";
    const LaneRoute route = select_lane(cfg);
    if (cfg->model == FVB_MODEL_PLUGIN)
    {
        // (the built-in spellings with the body's name in them)
        const std::string of = "<" + config_device_model(cfg) + "," + std::to_string(cfg->n_params);
        if (route.family == FVB_LANE_NOISE_PHIS)
            g_kernel_name = "lane_phis" + of + "," + std::to_string(route.pattern_n) + ">";
        else if (route.library())
            g_kernel_name = (route.family == FVB_LANE_NOISE_AR1 ? "lane_ar1" : "lane") + of + (cfg->need_f ? ",F>" : ">");
        else
            g_kernel_name = "wave<" + config_device_model(cfg) + ">";
        return g_kernel_name.c_str();
    }
    if (route.any() && g_variant != 2)
        return route.k.name;
    return "wave";
}

namespace
{
int run_device_as(const fvb_config *cfg, const void *data, const fvb_outputs *out, hipStream_t stream, int n_unmasked,
    int kernel_voxels, BlockSlot *slot = nullptr);
}

int32_t fabber_vb_run_device_ex(const fvb_config *cfg, const void *data, const fvb_outputs *out, void *stream_,
    int32_t n_unmasked)
{
    return run_device_as(cfg, data, out, (hipStream_t)stream_, n_unmasked, cfg ? cfg->n_voxels : 0);
}

namespace
{
// kernel_voxels: the voxel count the kernel choice (lane / wave) is made for - the whole problem's when
// cfg describes one block of it (fabber_vb_run_host_multi), so that every block runs the same code.
// slot: the kernels' work buffers (tiled series, saved state) come from the block's slot (pipelined host entry point)
// instead of the stream-ordered pool.
int run_device_as(const fvb_config *cfg, const void *data, const fvb_outputs *out, hipStream_t stream, int n_unmasked,
    int kernel_voxels, BlockSlot *slot)
{
    int rc = validate(cfg);
    if (rc)
        return rc;
    if (!out || !out->mvn)
        return fail(-20, "outputs.mvn is required");
    if (cfg->n_voxels == 0)
        return 0;
    if (!data)
        return fail(-21, "data is NULL");
    if (cfg->noise == FVB_NOISE_AR1 && n_unmasked != cfg->n_times)
        return fail(-15, "Masked time points are not supported for the AR noise model"); // noisemodel_ar.cc:351-355
    // A library body without init_mvn: the fit kernels know no model's InitVoxelPosterior. The kernel the library compiled
    // around the body's init_posterior writes the image (include/fabber_device_init_model.h); without such an entry the
    // image has to come from the model's host code, as for host-evaluated models.
    fvb_device_init_model init_entry;
    const bool init_on_device = cfg->model == FVB_MODEL_PLUGIN && !cfg->init_mvn && find_init_entry(cfg, &init_entry);
    if (cfg->model == FVB_MODEL_PLUGIN && !cfg->init_mvn && !init_on_device)
        return fail(-52, "host-evaluated models need the initial posterior as init_mvn (the model's InitVoxelPosterior runs on the host)");
    api_keep_pool_memory();
    KernelArgs ka;
    ka.cfg = *cfg;
    ka.out = *out;
    ka.data = data;
    ka.tiles = nullptr;
    ka.save = nullptr;
    ka.n_unmasked = n_unmasked;
    ka.residual_mode = g_residual_mode;
    ka.residual_tol = g_residual_tol;
    // The first two linearisations of a run evaluate the model pointwise (vb_lane_kernel.h, recentre). One would do
    // for a single exponential on the population (C2 against the oracle: median 1.5e-10 and 99th percentile 1.1e-8
    // either way, 8 % faster) but not on its worst voxel: 1.5e-6 against 1.05e-6, across the 1e-6 every strict
    // comparison holds without raising it (tools/measure/c2_precise_passes.py) - so two, for every model.
    ka.precise_passes = g_precise_passes >= 0 ? g_precise_passes : 2;

    fvb_config choice = *cfg;
    choice.n_voxels = kernel_voxels;
    const LaneRoute route = select_lane(&choice);
    const LaneKernelInfo &lk = route.k;
    const bool has_strided = route.has_strided, has_tiles = route.has_tiles;
    auto work_alloc = [&](void **p, size_t bytes) { return slot ? slot->take(p, bytes) : api_pool_alloc(p, bytes, stream); };
    // (a work buffer like the tiles: the block's slot on the pipelined host path - every block initialises its own columns -
    // the stream-ordered pool otherwise; written on the run's stream ahead of the kernels that read it)
    double *init_image = nullptr;
    if (init_on_device)
    {
        const size_t rows = (size_t)fabber_vb_mvn_rows(cfg->n_params + noise_outputs(cfg));
        FVB_HIP_CHECK(work_alloc((void **)&init_image, sizeof(double) * rows * (size_t)cfg->n_voxels));
        if ((rc = launch_init_entry(init_entry, cfg, data, init_image, stream)) != 0)
            return rc;
        ka.cfg.init_mvn = init_image;
    }
    if (route.any())
    {
        if (needs_save(cfg))
            FVB_HIP_CHECK(work_alloc((void **)&ka.save, sizeof(double) * (size_t)lk.save_rows * cfg->n_voxels));
        int feed = LANE_FEED_STRIDED;
        void *tiles = nullptr;
        // White noise, no masked timepoints: the series is re-laid per wavefront once (one read and one
        // write of the image) and every pass of the voxel loop streams that block (vb_lane_kernel.h).
        // (the AR(1) kernels exist for the tiled series only)
        if (has_tiles && (!has_strided || (n_unmasked == cfg->n_times && g_residual_mode != 1 && g_tiled)))
        {
            const int V = cfg->n_voxels, T = cfg->n_times;
            const unsigned rgrid = (unsigned)((V + 255) / 256);
            if (cfg->data_f64)
            {
                FVB_HIP_CHECK(work_alloc(&tiles, Tile<double>::bytes(V, T)));
                hipLaunchKernelGGL(retile_series<double>, dim3(rgrid), dim3(256), 0, stream, (const double *)data, (double *)tiles, V, T);
                feed = LANE_FEED_TILES_F64;
            }
            else
            {
                FVB_HIP_CHECK(work_alloc(&tiles, Tile<float>::bytes(V, T)));
                hipLaunchKernelGGL(retile_series<float>, dim3(rgrid), dim3(256), 0, stream, (const float *)data, (float *)tiles, V, T);
                feed = LANE_FEED_TILES_F32;
            }
            FVB_HIP_CHECK(hipGetLastError());
            ka.tiles = tiles;
        }
        // (the several-precisions kernels keep the T class bytes of the noise pattern in dynamic LDS)
        const size_t lds = (cfg->noise == FVB_NOISE_WHITE && cfg->n_phis > 1) ? (size_t)((cfg->n_times + 15) & ~15) : 0;
        const bool counting = cfg->convergence == FVB_CONV_MAXITS;
        if (route.library()) // the kernels live in the library's code object: its launcher starts the one for this feed
        {
            char msg[512];
            msg[0] = 0;
            // (the class bytes of a pattern kernel are sized here and nowhere else: the count travels in the call)
            rc = route.noise_launch ? route.noise_launch(&ka, route.family, route.pattern_n, feed, (uint32_t)lds, (void *)stream, msg, (int32_t)sizeof(msg))
                                    : route.launch(&ka, feed, counting ? 1 : 0, (void *)stream, msg, (int32_t)sizeof(msg));
            if (rc)
                g_last_error = msg;
        }
        else
            rc = launch_lane_kernel(lk, ka, feed, counting, lds, stream, g_last_error);
        if (rc)
            return rc;
        for (void *work : { tiles, (void *)ka.save, (void *)init_image })
            if (work && !slot)
                FVB_HIP_CHECK(api_pool_free(work, stream));
        return 0;
    }
    if (cfg->model == FVB_MODEL_PLUGIN) // the kernels live in the library's code object: its launcher starts them
    {
        fvb_device_model body;
        if (!find_wave_body(config_device_model(cfg), &body))
            return fail(-16, "no device model '" + config_device_model(cfg) + "' is registered (fabber_vb_register_device_model)");
        char msg[512];
        msg[0] = 0;
        rc = body.launch(&ka, (void *)stream, msg, (int32_t)sizeof(msg));
        if (rc)
            return fail(rc, msg);
        if (init_image && !slot)
            FVB_HIP_CHECK(api_pool_free(init_image, stream));
        return 0;
    }
    return launch_wave_kernel(ka, stream, g_last_error);
}
} // namespace

int32_t fabber_vb_run_device(const fvb_config *cfg, const void *data, const fvb_outputs *out, void *stream)
{
    // The number of unmasked timepoints is needed as a scalar by the kernels; phi_index is a
    // device pointer here, so read it back (n_times bytes, once per call).
    int n_unmasked = cfg ? cfg->n_times : 0;
    if (cfg && cfg->phi_index && cfg->n_times > 0)
    {
        std::vector<uint8_t> h(cfg->n_times);
        FVB_HIP_CHECK(hipMemcpyAsync(h.data(), cfg->phi_index, h.size(), hipMemcpyDeviceToHost, (hipStream_t)stream));
        FVB_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
        n_unmasked = count_unmasked((size_t)cfg->n_times, h.data());
    }
    return fabber_vb_run_device_ex(cfg, data, out, stream, n_unmasked);
}

namespace
{
// Voxels [v0, v1) of a host-resident problem on one device: the block's columns of every [row][voxel]
// image go up and down as 2-D copies (row pitch = the caller's n_voxels), the kernels see a problem of
// v1 - v0 voxels. Runs on `stream`; returns after the block's results are in the caller's arrays.
// The three stages of a block: in (allocate, upload), fit (the kernels), out (download). They may run on three
// different streams - the pipelined host entry point below uploads block b + 1 and downloads block b - 1 while block
// b is being fitted - ordered by the events up_done and fit_done.
struct HostBlock
{
    const fvb_config *cfg = nullptr;
    const void *data = nullptr;
    const fvb_outputs *out = nullptr;
    int v0 = 0, v1 = 0, kernel_voxels = 0;
    StagedProblem staged;
    hipEvent_t up_done = nullptr, fit_done = nullptr;
    BlockSlot *slot = nullptr; // pipelined entry point: where every device buffer of the block comes from
    ~HostBlock()
    {
        if (slot)
            slot->reset(); // (the owner destroys a block only after its work has been seen to finish)
        if (up_done)
            (void)hipEventDestroy(up_done);
        if (fit_done)
            (void)hipEventDestroy(fit_done);
    }
    int stage_in(hipStream_t stream)
    {
        const int rc = staged.stage_in(cfg, data, out, (size_t)fabber_vb_mvn_rows(cfg->n_params + noise_outputs(cfg)), (size_t)v0, (size_t)v1,
            stream, from_slot(slot), STAGE_VB);
        if (rc)
            return rc;
        FVB_HIP_CHECK(hipEventCreateWithFlags(&up_done, hipEventDisableTiming));
        FVB_HIP_CHECK(hipEventRecord(up_done, stream));
        return 0;
    }
    int fit(hipStream_t stream, int n_unmasked)
    {
        FVB_HIP_CHECK(hipStreamWaitEvent(stream, up_done, 0));
        int rc = run_device_as(&staged.d, staged.b_data.p, &staged.dout, stream, n_unmasked, kernel_voxels, slot);
        if (rc)
            return rc;
        FVB_HIP_CHECK(hipEventCreateWithFlags(&fit_done, hipEventDisableTiming));
        FVB_HIP_CHECK(hipEventRecord(fit_done, stream));
        return 0;
    }
    // returns after the block's results are in the caller's arrays (bounce: see StagedProblem::stage_out)
    int stage_out(hipStream_t stream, void *bounce = nullptr)
    {
        FVB_HIP_CHECK(hipStreamWaitEvent(stream, fit_done, 0));
        return staged.stage_out(out, stream, bounce);
    }
};

int run_host_block(const fvb_config *cfg, const void *data, const fvb_outputs *out, int device, int v0, int v1,
    hipStream_t stream, int kernel_voxels)
{
    FVB_HIP_CHECK(hipSetDevice(device));
    if (v1 <= v0)
        return 0;
    HostBlock b;
    b.cfg = cfg;
    b.data = data;
    b.out = out;
    b.v0 = v0;
    b.v1 = v1;
    b.kernel_voxels = kernel_voxels;
    int rc = b.stage_in(stream);
    if (rc == 0)
        rc = b.fit(stream, count_unmasked((size_t)cfg->n_times, cfg->phi_index));
    if (rc == 0)
        rc = b.stage_out(stream);
    if (rc)
        (void)hipStreamSynchronize(stream); // (before the block's buffers go back to the pool)
    return rc;
}

// The whole problem through host pointers on one device, as a PIPELINE over blocks of voxels: while block b is being
// fitted, block b + 1 goes up and block b - 1 comes down (three streams; the caller's buffers are pageable, so a copy
// holds the host thread that issued it: this thread uploads and launches, a second one downloads). What a voxel gets
// depends on nothing but that voxel, and every block runs the kernel the whole problem would, so the result is the
// one-block run's bit for bit (tests/test_multi_device.py). C3 (1e6 voxels, 400 MB up, 176 MB down): the sum of its
// parts was 7.5 + 15.2 + 3.3 ms = 28 - 29 ms with overheads; piped 25 - 27 ms. What keeps it from 1.9 + 15.2 + 0.8 ms
// (rocprofv3 --kernel-trace --memory-copy-trace of one call, profiles/r3_host_pipeline.md): the runtime takes a 2-D
// copy from pageable memory as gather -> DMA at 57 GB/s -> a blit KERNEL that has to find room between the resident
// wavefronts of the fit (1.7 - 2.6 ms per block, and the fit of a block 25 % longer while it runs). Tried and
// dropped: gathering the rows into pinned slots with 12 host threads and one DMA per slot - the host's own memcpy
// (~20 GB/s) is then on the critical path: 32 - 37 ms. A caller that keeps its buffers can take the copies off the
// host altogether: fabber_vb_pin_host_buffer (below) - the same calls then are asynchronous rectangle DMAs.
// The four streams of a pipelined call (and a pinned bounce buffer for the blocks' small result arrays) are kept between
// calls: creating and destroying them was 4 - 5 ms of a 23 ms call (hipStreamCreateWithFlags 0.45 - 0.6 ms each,
// hipStreamDestroy 0.5 - 1.2 ms each: rocprofv3 --hip-runtime-trace, tools/measure/host_timeline.sh). A call takes a
// set of its device from the cache or makes one; fabber_vb_release_cached_memory destroys the idle ones.
struct PipeStreams
{
    int device = -1;
    hipStream_t up = nullptr, fit[2] = { nullptr, nullptr }, down = nullptr;
    void *bounce = nullptr; // pinned host memory
    size_t bounce_bytes = 0;
    BlockSlot slots[3];     // device memory of the (at most three) blocks in flight
    int create(int dev)
    {
        device = dev;
        FVB_HIP_CHECK(hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
        FVB_HIP_CHECK(hipStreamCreateWithFlags(&fit[0], hipStreamNonBlocking));
        FVB_HIP_CHECK(hipStreamCreateWithFlags(&fit[1], hipStreamNonBlocking));
        FVB_HIP_CHECK(hipStreamCreateWithFlags(&down, hipStreamNonBlocking));
        return 0;
    }
    int need_bounce(size_t bytes)
    {
        if (bytes <= bounce_bytes)
            return 0;
        if (bounce)
            (void)hipHostFree(bounce);
        bounce = nullptr;
        bounce_bytes = 0;
        FVB_HIP_CHECK(hipHostMalloc(&bounce, bytes, hipHostMallocDefault));
        bounce_bytes = bytes;
        return 0;
    }
    void destroy()
    {
        for (hipStream_t s : { up, fit[0], fit[1], down })
            if (s)
                (void)hipStreamDestroy(s);
        if (bounce)
            (void)hipHostFree(bounce);
        for (BlockSlot &sl : slots)
            sl.destroy();
        up = fit[0] = fit[1] = down = nullptr;
        bounce = nullptr;
        bounce_bytes = 0;
    }
};
struct PipeStreamCache
{
    std::mutex lock;
    std::vector<PipeStreams> idle;
};
static PipeStreamCache &pipe_stream_cache()
{
    static PipeStreamCache c;
    return c;
}
static int acquire_pipe_streams(int device, PipeStreams &ps)
{
    {
        PipeStreamCache &c = pipe_stream_cache();
        std::lock_guard<std::mutex> hold(c.lock);
        for (size_t i = 0; i < c.idle.size(); i++)
            if (c.idle[i].device == device)
            {
                ps = c.idle[i];
                c.idle.erase(c.idle.begin() + (long)i);
                return 0;
            }
    }
    const int rc = ps.create(device);
    if (rc)
        ps.destroy();
    return rc;
}
static void release_pipe_streams(const PipeStreams &ps)
{
    PipeStreamCache &c = pipe_stream_cache();
    std::lock_guard<std::mutex> hold(c.lock);
    c.idle.push_back(ps);
}
void destroy_idle_pipe_streams()
{
    PipeStreamCache &c = pipe_stream_cache();
    std::lock_guard<std::mutex> hold(c.lock);
    int now = 0;
    (void)hipGetDevice(&now);
    for (PipeStreams &ps : c.idle)
    {
        if (hipSetDevice(ps.device) == hipSuccess)
            ps.destroy();
    }
    c.idle.clear();
    (void)hipSetDevice(now);
}

int run_host_pipelined(const fvb_config *cfg, const void *data, const fvb_outputs *out, int device, int block_voxels)
{
    FVB_HIP_CHECK(hipSetDevice(device));
    const int V = cfg->n_voxels;
    // The blocks: the upload is about twice as fast as the fit (56 GB/s of series against ~75 voxels/us on C3), so after
    // the first block the fits are what the call waits for - the first block is as small as fills the chip once (its
    // upload is the pipeline's fill, nothing overlaps it), the last one too (its download is the drain), the ones in
    // between the nominal size: a block more than twice its predecessor is still going up when that one's fit ends
    // (measured on C3, tools/measure/host_pipeline.py: 131072 / 262144 / 262144 / 213568 / 131072 voxels 23.1 ms,
    // four equal blocks 23.9, 131072 / 368960 / 368896 / 131072 25.1). FVB_HOST_BLOCK_SCHEDULE=a,b,c,... (voxels per
    // block, the last one takes the rest) overrides it for experiments.
    std::vector<int> bounds(1, 0);
    if (const char *sched = getenv("FVB_HOST_BLOCK_SCHEDULE"))
    {
        for (const char *p = sched; *p && bounds.back() < V;)
        {
            const int n = std::max(64, atoi(p) / 64 * 64);
            bounds.push_back(std::min(V, bounds.back() + n));
            while (*p && *p != ',')
                p++;
            if (*p == ',')
                p++;
        }
        if (bounds.back() < V)
            bounds.push_back(V);
    }
    else
    {
        const int edge = std::max(64, block_voxels / 2 / 64 * 64);
        if (V >= 2 * edge + block_voxels)
        {
            const int middle = (V - edge) / 64 * 64 - edge; // (every block but the last is whole wavefronts)
            bounds.push_back(edge);
            for (int done = 0; done < middle; done += block_voxels)
                bounds.push_back(edge + std::min(middle, done + block_voxels));
            bounds.push_back(V);
        }
        else
            for (int v = block_voxels; bounds.back() < V; v += block_voxels)
                bounds.push_back(std::min(V, v));
    }
    const int n_blocks = (int)bounds.size() - 1;
    const int n_unmasked = count_unmasked((size_t)cfg->n_times, cfg->phi_index);
    // (two streams take the blocks' kernels in turn: the first wavefronts of block b + 1 move into the SIMDs the last
    // stragglers of block b have left, instead of every block paying for its own tail)
    PipeStreams ps;
    {
        const int rc_streams = acquire_pipe_streams(device, ps);
        if (rc_streams)
            return rc_streams;
    }
    hipStream_t s_up = ps.up, s_fit[2] = { ps.fit[0], ps.fit[1] }, s_down = ps.down;
    {
        // the small result arrays of a block (F, history length, status, iterations) come down as ONE copy into pinned
        // memory and are handed out from there: four pageable copies of ~1 MB cost the download thread 0.15 - 0.3 ms each
        int widest = 0;
        for (int b = 0; b < n_blocks; b++)
            widest = std::max(widest, bounds[(size_t)b + 1] - bounds[(size_t)b]);
        const int rc_bounce = ps.need_bounce((size_t)widest * StagedProblem::SMALL_BYTES_PER_VOXEL + 64);
        if (rc_bounce)
        {
            ps.destroy();
            return rc_bounce;
        }
    }
    std::vector<std::unique_ptr<HostBlock> > blocks((size_t)n_blocks);
    // blocks whose results are down: their buffers go back to the pool on a thread of their own (hipFreeAsync of a
    // block's buffers took 0.4 - 1.0 ms of the download thread per block)
    std::vector<std::unique_ptr<HostBlock> > finished;
    bool no_more_finished = false;
    std::mutex lock;
    std::condition_variable cv;
    int launched = 0;       // blocks whose fit has been enqueued
    int released = 0;       // blocks whose buffers have gone back to the pool
    bool abandoned = false; // the uploading side failed: no more blocks will come
    int rc_down = 0;
    std::string err_down;
    std::thread downloader([&] {
        if (hipSetDevice(device) != hipSuccess)
        {
            std::unique_lock<std::mutex> hold(lock);
            rc_down = -32;
            err_down = "cannot select the device in the download thread";
            cv.notify_all();
            return;
        }
        for (int b = 0; b < n_blocks; b++)
        {
            {
                std::unique_lock<std::mutex> hold(lock);
                cv.wait(hold, [&] { return launched > b || abandoned; });
                if (launched <= b)
                    return;
            }
            const int rc = blocks[(size_t)b]->stage_out(s_down, ps.bounce);
            std::unique_lock<std::mutex> hold(lock);
            if (rc && rc_down == 0)
            {
                rc_down = rc;
                err_down = g_last_error; // thread-local: carry it to the caller's thread
            }
            finished.push_back(std::move(blocks[(size_t)b])); // (to the reaper: at most three blocks are resident)
            cv.notify_all();
        }
    });
    std::thread reaper([&] {
        (void)hipSetDevice(device);
        for (;;)
        {
            std::unique_ptr<HostBlock> blk;
            {
                std::unique_lock<std::mutex> hold(lock);
                cv.wait(hold, [&] { return !finished.empty() || no_more_finished; });
                if (finished.empty())
                    return;
                blk = std::move(finished.front());
                finished.erase(finished.begin());
            }
            blk.reset(); // its buffers go back to the pool
            std::unique_lock<std::mutex> hold(lock);
            released++;
            cv.notify_all();
        }
    });
    int rc = 0;
    for (int b = 0; b < n_blocks && rc == 0; b++)
    {
        {
            // at most three blocks hold device buffers at once (with copies that really are asynchronous - buffers the
            // caller pinned - this loop would otherwise stage the whole problem before the first download ends)
            std::unique_lock<std::mutex> hold(lock);
            cv.wait(hold, [&] { return b - released < 3 || rc_down != 0; });
        }
        std::unique_ptr<HostBlock> blk(new HostBlock);
        blk->cfg = cfg;
        blk->data = data;
        blk->out = out;
        blk->v0 = bounds[(size_t)b];
        blk->v1 = bounds[(size_t)b + 1];
        blk->kernel_voxels = V;
        blk->slot = &ps.slots[b % 3]; // (free: block b - 3 has been reaped, see the wait above)
        rc = blk->stage_in(s_up);
        if (rc == 0)
            rc = blk->fit(s_fit[b & 1], n_unmasked);
        std::unique_lock<std::mutex> hold(lock);
        if (rc == 0)
        {
            blocks[(size_t)b] = std::move(blk);
            launched = b + 1;
        }
        else
        {
            (void)hipDeviceSynchronize(); // (before the failed block's buffers go back to the pool)
            abandoned = true;
        }
        cv.notify_all();
    }
    downloader.join();
    (void)hipStreamSynchronize(s_up);
    (void)hipStreamSynchronize(s_fit[0]);
    (void)hipStreamSynchronize(s_fit[1]);
    (void)hipStreamSynchronize(s_down);
    {
        std::unique_lock<std::mutex> hold(lock);
        no_more_finished = true;
        cv.notify_all();
    }
    reaper.join();
    blocks.clear();
    release_pipe_streams(ps);
    if (rc)
        return rc;
    if (rc_down)
        return fail(rc_down, err_down);
    return 0;
}
} // namespace

int32_t fabber_vb_run_host(const fvb_config *cfg, const void *data, const fvb_outputs *out, int32_t device)
{
    int rc = validate(cfg);
    if (rc)
        return rc;
    if (!out || !out->mvn)
        return fail(-20, "outputs.mvn is required");
    if (fabber_vb_device_count() <= 0)
        return fail(-30, "no HIP device available (the VB engine has no CPU fallback)");
    // large problems on a throughput (lane) kernel: upload, fit and download overlap block by block. A block holds
    // as many voxels as fill the chip twice (256 CUs x 4 SIMDs x 2 waves x 64 lanes = 131072): smaller ones leave
    // SIMDs idle in every block's tail, larger ones lengthen the pipeline's fill and drain.
    int block = 262144;
    if (const char *e = getenv("FVB_HOST_BLOCK_VOXELS")) // (0 = one block, the round-2 behaviour)
        block = atoi(e) / 64 * 64;
    fvb_config choice = *cfg;
    // (a library model's wave kernels take what they need from the block alone, like the lane kernels: piped as well)
    if (block > 0 && cfg->n_voxels >= 2 * block
        && (select_lane(&choice).any() || cfg->model == FVB_MODEL_PLUGIN))
        return run_host_pipelined(cfg, data, out, device, block);
    return run_host_block(cfg, data, out, device, 0, cfg->n_voxels, nullptr, cfg->n_voxels);
}

int32_t fabber_vb_run_host_multi(const fvb_config *cfg, const void *data, const fvb_outputs *out,
    const int32_t *devices, int32_t n_devices, fvb_summary *summary)
{
    int rc = validate(cfg);
    if (rc)
        return rc;
    if (!out || !out->mvn)
        return fail(-20, "outputs.mvn is required");
    const int visible = fabber_vb_device_count();
    if (visible <= 0)
        return fail(-30, "no HIP device available (the VB engine has no CPU fallback)");
    std::vector<int> devs;
    if (devices)
    {
        if (n_devices <= 0)
            return fail(-31, "empty device list");
        for (int i = 0; i < n_devices; i++)
        {
            if (devices[i] < 0 || devices[i] >= visible)
                return fail(-31, "device index " + std::to_string(devices[i]) + " out of range (" + std::to_string(visible) + " visible)");
            devs.push_back(devices[i]);
        }
    }
    else
        for (int i = 0; i < visible; i++)
            devs.push_back(i);
    const int n = (int)devs.size();
    const long long V = cfg->n_voxels;
    // contiguous blocks, cut on multiples of 64 voxels (a wavefront of the lane kernels) so that a
    // voxel shares its wavefront with the same neighbours as in a one-device run
    std::vector<int> cut(n + 1, 0);
    for (int i = 1; i < n; i++)
        cut[i] = (int)std::min<long long>(V, ((V * i / n + 63) / 64) * 64);
    cut[n] = (int)V;
    std::vector<int> rcs(n, 0);
    std::vector<std::string> errs(n);
    std::vector<std::thread> pool;
    // (a device listed several times - a rehearsal of the N-block path on one GPU - takes its blocks one after the other:
    // several streams on one device's stream-ordered pool are what ROCm 7.2's runtime does not keep apart)
    std::vector<std::mutex> one_at_a_time((size_t)visible);
    for (int i = 0; i < n; i++)
        pool.emplace_back([&, i] {
            std::lock_guard<std::mutex> turn(one_at_a_time[(size_t)devs[i]]);
            hipStream_t st = nullptr;
            if (hipSetDevice(devs[i]) != hipSuccess || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess)
            {
                rcs[i] = -32;
                errs[i] = "cannot create a stream on device " + std::to_string(devs[i]);
                return;
            }
            // every block runs the kernel the whole problem would (kernel choice depends on the voxel count)
            rcs[i] = run_host_block(cfg, data, out, devs[i], cut[i], cut[i + 1], st, cfg->n_voxels);
            if (rcs[i])
                errs[i] = g_last_error; // thread-local: carry it to the caller's thread
            (void)hipStreamDestroy(st);
        });
    for (auto &t : pool)
        t.join();
    for (int i = 0; i < n; i++)
        if (rcs[i])
            return fail(rcs[i], "block " + std::to_string(i) + " (device " + std::to_string(devs[i]) + "): " + errs[i]);
    if (summary)
    {
        summary->sum_free_energy = 0;
        summary->sum_iterations = 0;
        summary->bad_voxels = 0;
        for (long long v = 0; v < V; v++)
        {
            const bool ok = !out->status || (out->status[v] & 0xff) == 0;
            if (out->status && !ok)
                summary->bad_voxels++;
            if (out->free_energy && ok)
                summary->sum_free_energy += out->free_energy[v];
            if (out->iterations)
                summary->sum_iterations += out->iterations[v];
        }
    }
    return 0;
}

int32_t fabber_vb_register_device_results_model(const fvb_device_results_model *model)
{
    return DeviceRegistry<fvb_device_results_model>::instance().add(model);
}

int32_t fabber_vb_unregister_device_results_model(const char *name)
{
    return DeviceRegistry<fvb_device_results_model>::instance().remove(name, 0);
}

int32_t fabber_vb_device_results_model_count(void)
{
    return DeviceRegistry<fvb_device_results_model>::instance().count();
}

const char *fabber_vb_device_results_model_name(int32_t i)
{
    return DeviceRegistry<fvb_device_results_model>::instance().name(i);
}

const char *fabber_vb_postproc_kernel_name(const fvb_config *cfg)
{
    if (validate(cfg, true, true) != 0)
        return "";
    g_postproc_kernel_name = select_postproc(cfg).name;
    return g_postproc_kernel_name.c_str();
}

int32_t fabber_vb_postproc_device(const fvb_config *cfg, const void *data, const double *mvn, const fvb_postproc *pp,
    void *stream)
{
    int rc = validate(cfg, true, true); // the output images do not depend on the prior types
    if (rc)
        return rc;
    if (!mvn || !pp)
        return fail(-22, "mvn / postproc outputs are NULL");
    if ((pp->residuals) && !data)
        return fail(-21, "residuals need the data");
    const bool want_fit = pp->modelfit || pp->residuals;
    const PostprocRoute route = select_postproc(cfg);
    if (want_fit && !route.fit)
        return fail(-85, "model fit / residuals of the device model '" + config_device_model(cfg)
                + "': its library registered no result-image kernel for it (FABBER_DEVICE_RESULTS_MODEL in "
                  "include/fabber_device_results_model.h); the engine cannot evaluate the body itself");
    if (cfg->n_voxels == 0)
        return 0;
    if (want_fit && route.library)
    {
        char err[256] = "";
        rc = route.library(cfg, data, mvn, pp, noise_outputs(cfg), stream, err, (int32_t)sizeof(err));
        return rc ? fail(rc, "result-image kernel of the device model '" + config_device_model(cfg) + "': " + err) : 0;
    }
    // (means, variances and noise images need no model: the engine's kernel, whatever the model)
    FVB_HIP_CHECK(launch_postproc<BuiltinEval>(*cfg, data, mvn, *pp, noise_outputs(cfg), (hipStream_t)stream));
    return 0;
}

int32_t fabber_vb_postproc_host(const fvb_config *cfg, const void *data, const double *mvn, const fvb_postproc *pp,
    int32_t device)
{
    int rc = validate(cfg, true, true);
    if (rc)
        return rc;
    if (fabber_vb_device_count() <= 0)
        return fail(-30, "no HIP device available (the VB engine has no CPU fallback)");
    FVB_HIP_CHECK(hipSetDevice(device));
    const size_t V = (size_t)cfg->n_voxels, T = (size_t)cfg->n_times;
    if (V == 0)
        return 0;
    const int P = cfg->n_params, N = noise_outputs(cfg);
    const int rows = fabber_vb_mvn_rows(P + N);
    const size_t esz = cfg->data_f64 ? 8 : 4;
    fvb_config d = *cfg;
    DevMem b_data, b_design, b_consts, b_supp, b_mvn;
    DeviceParamTable ptable;
    if (cfg->params_ext)
    {
        fvb_config no_images = *cfg; // (the images of image priors play no part in the result images)
        fvb_param_table t = *cfg->params_ext;
        t.image_prior = nullptr;
        std::vector<int32_t> types((size_t)P, FVB_PRIOR_NORMAL);
        t.prior_type = types.data();
        no_images.params_ext = &t;
        if ((rc = ptable.upload(&no_images, 0, V, nullptr)) != 0)
            return rc;
        d.params_ext = ptable.device;
    }
    if (data && (rc = upload_array(b_data, data, T * V * esz, nullptr)) != 0)
        return rc;
    if (cfg->design)
    {
        if ((rc = upload_array(b_design, cfg->design, sizeof(double) * T * P, nullptr)) != 0)
            return rc;
        d.design = (const double *)b_design.p;
    }
    d.model_consts = nullptr; // (a host pointer: the kernel of a library's body reads the device copy, no other kernel reads any)
    if (cfg->model == FVB_MODEL_PLUGIN && cfg->model_consts && cfg->n_model_consts > 0)
    {
        if ((rc = upload_array(b_consts, cfg->model_consts, sizeof(double) * (size_t)cfg->n_model_consts, nullptr)) != 0)
            return rc;
        d.model_consts = (const double *)b_consts.p;
    }
    d.model_supp = nullptr; // (the same for the voxels' supplementary data, [n_model_supp][V])
    if (cfg->model == FVB_MODEL_PLUGIN && cfg->model_supp && cfg->n_model_supp > 0)
    {
        if ((rc = upload_array(b_supp, cfg->model_supp, sizeof(double) * (size_t)cfg->n_model_supp * V, nullptr)) != 0)
            return rc;
        d.model_supp = (const double *)b_supp.p;
    }
    FVB_HIP_CHECK(b_mvn.alloc(sizeof(double) * rows * V));
    {
        // Only the rows the kernel reads go up: the means (contiguous) and, where a variance is asked for, the diagonal of
        // the covariance - for C3's mean images 40 MB of the 168 MB image (3 ms of a 30 ms fabber_dorun at PCIe rate).
        const int n = P + N, nCov = n * (n + 1) / 2;
        const size_t row = sizeof(double) * V;
        FVB_HIP_CHECK(hipMemcpy((char *)b_mvn.p + (size_t)nCov * row, (const char *)mvn + (size_t)nCov * row, (size_t)n * row, hipMemcpyHostToDevice));
        if (pp->var || pp->std || pp->zstat || pp->noise_std)
            for (int q = 0; q < n; q++)
            {
                const size_t r = (size_t)(q * (q + 1) / 2 + q);
                FVB_HIP_CHECK(hipMemcpy((char *)b_mvn.p + r * row, (const char *)mvn + r * row, row, hipMemcpyHostToDevice));
            }
        else // (the kernel loads the variance beside the mean whatever is asked for: give it something defined)
            for (int q = 0; q < n; q++)
                FVB_HIP_CHECK(hipMemsetAsync((char *)b_mvn.p + (size_t)(q * (q + 1) / 2 + q) * row, 0, row, nullptr));
    }
    struct Item
    {
        double *const *host;
        double **dev;
        size_t rows;
    };
    fvb_postproc dpp;
    memset(&dpp, 0, sizeof(dpp));
    Item items[8] = { { &pp->mean, &dpp.mean, (size_t)P }, { &pp->var, &dpp.var, (size_t)P },
        { &pp->std, &dpp.std, (size_t)P }, { &pp->zstat, &dpp.zstat, (size_t)P }, { &pp->modelfit, &dpp.modelfit, T },
        { &pp->residuals, &dpp.residuals, T }, { &pp->noise_mean, &dpp.noise_mean, (size_t)N },
        { &pp->noise_std, &dpp.noise_std, (size_t)N } };
    DevMem bufs[8];
    for (int i = 0; i < 8; i++)
        if (*items[i].host)
        {
            FVB_HIP_CHECK(bufs[i].alloc(sizeof(double) * items[i].rows * V));
            *items[i].dev = (double *)bufs[i].p;
        }
    rc = fabber_vb_postproc_device(&d, data ? b_data.p : nullptr, (const double *)b_mvn.p, &dpp, nullptr);
    if (rc)
        return rc;
    FVB_HIP_CHECK(hipDeviceSynchronize());
    for (int i = 0; i < 8; i++)
        if (*items[i].host)
            FVB_HIP_CHECK(hipMemcpy(*items[i].host, *items[i].dev, sizeof(double) * items[i].rows * V, hipMemcpyDeviceToHost));
    return 0;
}

int32_t fabber_vb_register_device_init_model(const fvb_device_init_model *model)
{
    return DeviceRegistry<fvb_device_init_model>::instance().add(model);
}

int32_t fabber_vb_unregister_device_init_model(const char *name)
{
    return DeviceRegistry<fvb_device_init_model>::instance().remove(name, 0);
}

int32_t fabber_vb_device_init_model_count(void)
{
    return DeviceRegistry<fvb_device_init_model>::instance().count();
}

const char *fabber_vb_device_init_model_name(int32_t i)
{
    return DeviceRegistry<fvb_device_init_model>::instance().name(i);
}

namespace
{
thread_local std::string g_init_kernel_name;
// (the prior types of spatial VB are as good as any other here; a parameter table has none of them)
int validate_for_init(const fvb_config *cfg)
{
    return validate(cfg, !(cfg && cfg->params_ext));
}
} // namespace

const char *fabber_vb_init_posterior_kernel_name(const fvb_config *cfg)
{
    if (validate_for_init(cfg) != 0 || cfg->init_mvn || !find_init_entry(cfg))
        return "";
    g_init_kernel_name = "init<" + config_device_model(cfg) + ">";
    return g_init_kernel_name.c_str();
}

int32_t fabber_vb_init_posterior_device(const fvb_config *cfg, const void *data, double *init_mvn_out, void *stream)
{
    int rc = validate_for_init(cfg);
    if (rc)
        return rc;
    if (!init_mvn_out)
        return fail(-22, "the image to write (init_mvn_out) is NULL");
    if (cfg->model != FVB_MODEL_PLUGIN)
        return fail(-95, "the initial posterior of a built-in model is set inside its fit kernels: there is no image to compute "
                         "(fabber_vb_init_posterior_* is for the device body of a model library, FVB_MODEL_PLUGIN)");
    fvb_device_init_model entry;
    if (!find_init_entry(cfg, &entry))
        return fail(-95, "initial posterior of the device model '" + config_device_model(cfg)
                + "': its library registered no initial-posterior kernel for it (FABBER_DEVICE_INIT_MODEL in "
                  "include/fabber_device_init_model.h); the model's InitVoxelPosterior runs on the host");
    if (cfg->n_voxels == 0)
        return 0;
    if (!data)
        return fail(-21, "data is NULL");
    return launch_init_entry(entry, cfg, data, init_mvn_out, (hipStream_t)stream);
}

int32_t fabber_vb_init_posterior_host(const fvb_config *cfg, const void *data, double *init_mvn_out, int32_t device)
{
    int rc = validate_for_init(cfg);
    if (rc)
        return rc;
    if (cfg->model != FVB_MODEL_PLUGIN || !find_init_entry(cfg)) // (the refusals of the device entry point, before any upload)
        return fabber_vb_init_posterior_device(cfg, data, init_mvn_out, nullptr);
    if (!init_mvn_out)
        return fail(-22, "the image to write (init_mvn_out) is NULL");
    if (fabber_vb_device_count() <= 0)
        return fail(-30, "no HIP device available (the VB engine has no CPU fallback)");
    FVB_HIP_CHECK(hipSetDevice(device));
    const size_t V = (size_t)cfg->n_voxels;
    if (V == 0)
        return 0;
    if (!data)
        return fail(-21, "data is NULL");
    // the series, the constants and the image priors (or the parameter table) go up as for a fit; the staged problem's
    // result image has the rows of the initial posterior: the kernel writes it there
    const size_t rows = (size_t)fabber_vb_mvn_rows(cfg->n_params + noise_outputs(cfg));
    fvb_outputs none;
    memset(&none, 0, sizeof(none));
    StagedProblem staged;
    if ((rc = staged.stage_in(cfg, data, &none, rows, 0, V, nullptr, from_pool(), STAGE_PRIORS)) != 0)
        return rc;
    if ((rc = fabber_vb_init_posterior_device(&staged.d, staged.b_data.p, staged.dout.mvn, nullptr)) != 0)
        return rc;
    FVB_HIP_CHECK(hipMemcpy(init_mvn_out, staged.dout.mvn, sizeof(double) * rows * V, hipMemcpyDeviceToHost));
    return 0;
}

// ---- host-compiled twins of device building blocks, for unit tests without a GPU --------------
int32_t fabber_vb_convergence_trace(int32_t conv, int32_t max_iterations, int32_t max_trials, double min_fchange,
    const double *F, int32_t nF, int32_t *done, int32_t *save, int32_t *revert, double *alpha, int32_t stop_at_done)
{
    ConvState c;
    conv_init(c, conv, max_iterations, max_trials, min_fchange);
    conv_reset(c);
    int n = 0;
    for (int i = 0; i < nF; i++)
    {
        bool d = conv_test(c, F[i]);
        done[i] = d;
        save[i] = conv_need_save(c);
        revert[i] = conv_need_revert(c);
        alpha[i] = conv_lm_alpha(c);
        n++;
        if (d && stop_at_done)
            break;
    }
    return n;
}

double fabber_vb_gammaln(double x)
{
    return gammaln(x);
}
double fabber_vb_digamma(double x)
{
    return digamma(x);
}
double fabber_vb_exp_acc(double x) // (the host twin of the kernels' half-ulp exp, for tests/test_math_host.py)
{
    return exp_acc(x);
}
double fabber_vb_transform(int32_t which, int32_t tr, double x)
{
    switch (which)
    {
    case 0:
        return to_model(tr, x);
    case 1:
        return to_fabber(tr, x);
    case 2:
        return to_model_var(tr, x);
    default:
        return to_fabber_var(tr, x);
    }
}

// The same building blocks evaluated ON THE DEVICE (tests/test_hip_parity.py: the kernels are compiled with
// contraction allowed, so the error-free transforms inside exp_acc and the frexp-product log-determinant are checked
// as the device compiles them, not only through their host twin). what: 0 exp_acc with its table in LDS as the
// kernels keep it, 1 the device library's exp, 2 mvn_invert<4> of the packed 4 x 4 matrix at in[10 i ..]: out[11 i ..]
// = the packed inverse and log|det|. Host pointers; n values / matrices.
int32_t fabber_vb_device_math(int32_t what, int32_t n, const double *in, double *out)
{
    if (fabber_vb_device_count() <= 0)
        return fail(-30, "no HIP device available");
    if (n <= 0 || !in || !out || what < 0 || what > 2)
        return fail(-60, "fabber_vb_device_math: bad arguments");
    const size_t n_in = (size_t)n * (what == 2 ? 10 : 1), n_out = (size_t)n * (what == 2 ? 11 : 1);
    double *d_in = nullptr, *d_out = nullptr;
    FVB_HIP_CHECK(hipMalloc(&d_in, sizeof(double) * n_in));
    FVB_HIP_CHECK(hipMalloc(&d_out, sizeof(double) * n_out));
    FVB_HIP_CHECK(hipMemcpy(d_in, in, sizeof(double) * n_in, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(device_math_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr, what, n, (const double *)d_in, d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpy(out, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return e == hipSuccess ? 0 : fail(-100 - (int)e, hipGetErrorString(e));
}

// Host twin of the in-register LDL^T inverse for P = 1..6 (unit test of vb_math.h)
int32_t fabber_vb_ldl_inverse(int32_t P, const double *packed, double *inv_packed, double *logabs, int32_t *sign)
{
    bool ok = false;
    double la = 0;
    int sg = 1;
#define FVB_LDL_CASE(PP)                                                                                     \
    case PP:                                                                                                 \
    {                                                                                                        \
        double a[PP * (PP + 1) / 2], r[PP * (PP + 1) / 2];                                                   \
        for (int i = 0; i < PP * (PP + 1) / 2; i++)                                                          \
            a[i] = packed[i];                                                                                \
        ok = mvn_invert<PP>(a, r, la, sg);                                                                   \
        for (int i = 0; i < PP * (PP + 1) / 2; i++)                                                          \
            inv_packed[i] = r[i];                                                                            \
        break;                                                                                               \
    }
    switch (P)
    {
        FVB_LDL_CASE(1)
        FVB_LDL_CASE(2)
        FVB_LDL_CASE(3)
        FVB_LDL_CASE(4)
        FVB_LDL_CASE(5)
        FVB_LDL_CASE(6)
    default:
        return -1;
    }
    if (logabs)
        *logabs = la;
    if (sign)
        *sign = sg;
    return ok ? 0 : 1;
}

} // extern "C"
