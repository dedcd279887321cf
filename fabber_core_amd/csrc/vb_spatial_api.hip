/*
 * vb_spatial_api.hip - host driver of spatial VB on one device: the iteration loop of Vb::DoCalculationsSpatial
 * (inference_vb.cc:605-725) as a sequence of launches on one stream. See vb_spatial.h for the kernels,
 * vb_spatial_plan.h for the planning (neighbour lists, level ordering, slab numbering), vb_spatial_geom.h for its
 * device variants and vb_spatial_multi.hip for one volume on several devices.
 */
#include "vb_spatial_geom.h"
#include "vb_device_registry.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

using namespace fvb;

// Which statistics a configuration's state image carries (vb_spatial_noise.h), or -1: no spatial kernels for it
int fvb::spatial_noise_kind(const fvb_config *cfg)
{
    if (cfg->noise == FVB_NOISE_WHITE)
        return cfg->n_phis == 1 ? FVB_SPNZ_WHITE : (cfg->n_phis == 2 ? FVB_SPNZ_PATTERN2 : (cfg->n_phis <= 4 ? FVB_SPNZ_PATTERN4 : (cfg->n_phis <= 8 ? FVB_SPNZ_PATTERN8 : -1)));
    if (cfg->noise == FVB_NOISE_AR1 && cfg->n_phis == 1 && cfg->ar_cross_terms == 0)
        return FVB_SPNZ_AR1;
    if (cfg->noise == FVB_NOISE_AR1 && cfg->n_phis == 2 && cfg->ar_cross_terms >= 0 && cfg->ar_cross_terms <= 2)
        return FVB_SPNZ_ARN2 + cfg->ar_cross_terms;
    return -1;
}
const char *const fvb::spatial_noise_refusal
    = "spatial VB runs white noise with up to 8 noise precisions and AR(1) noise with one or two echoes";
namespace fvb
{
// The spatial kernels of device bodies that model libraries have registered (include/fabber_device_spatial_model.h), by
// (name, parameter count).
template <> struct DeviceRegistryTraits<fvb_device_spatial_model>
{
    static constexpr const char *noun = "device spatial model", *is = "are";
    static constexpr int first_code = -75;
    static std::vector<DeviceStructSize> sizes(const fvb_device_spatial_model &m)
    {
        return { { "SpatialArgs", m.spatial_args_size, sizeof(SpatialArgs) } };
    }
    static const char *bad_params(const fvb_device_spatial_model &m)
    {
        return (m.n_params < 1 || m.n_params > 6) ? "the spatial kernels of a library body exist for 1 to 6" : nullptr;
    }
    static std::string entry(const std::string &name, int n_params)
    {
        return "spatial kernels of a device model named '" + name + "' with " + std::to_string(n_params) + " parameters";
    }
    static std::string absent(const std::string &name, int n_params)
    {
        return "no " + entry(name, n_params) + " are registered";
    }
};
// ... and the ones compiled around the noise policies beyond white noise with one precision
// (include/fabber_device_spatial_noise_model.h), by (name, parameter count): a registry of its own, an entry says which
// families its library compiled.
template <> struct DeviceRegistryTraits<fvb_device_spatial_noise_model>
{
    static constexpr const char *noun = "device spatial noise model", *is = "are";
    static constexpr int first_code = -65;
    static std::vector<DeviceStructSize> sizes(const fvb_device_spatial_noise_model &m)
    {
        return { { "SpatialArgs", m.spatial_args_size, sizeof(SpatialArgs) } };
    }
    static const char *bad_params(const fvb_device_spatial_noise_model &m)
    {
        if (m.n_params < 1 || m.n_params > 6)
            return "the spatial kernels of a library body exist for 1 to 6";
        if (m.families == 0 || (m.families & ~(FVB_SPATIAL_NOISE_AR1 | FVB_SPATIAL_NOISE_PHIS)) != 0)
            return "the families mask names none of FVB_SPATIAL_NOISE_AR1 and FVB_SPATIAL_NOISE_PHIS, or a family this engine does not know";
        return (m.state_rows_ar1 < 0 || m.state_rows_phis2 < 0 || m.state_rows_phis4 < 0) ? "a negative row count of the state image" : nullptr;
    }
    static std::string entry(const std::string &name, int n_params)
    {
        return "AR(1) / noise-pattern spatial kernels of a device model named '" + name + "' with " + std::to_string(n_params) + " parameters";
    }
    static std::string absent(const std::string &name, int n_params)
    {
        return "no " + entry(name, n_params) + " are registered";
    }
};
// ... and the two kernels of the wave-per-voxel family compiled around a body (include/fabber_device_spatial_wave_model.h),
// by name: the parameter count is a runtime value there. vb_spatial_wave.hip has the table and the layout these go with.
SpatialKernels get_spatial_kernels_wave_model(int P, bool need_f);
uint32_t spatial_wave_model_lds_probe();
size_t spatial_wave_layout_size(); // sizeof(WaveLayout)
template <> struct DeviceRegistryTraits<fvb_device_spatial_wave_model>
{
    static constexpr const char *noun = "device spatial wave model", *is = "are";
    static constexpr int first_code = -35;
    static std::vector<DeviceStructSize> sizes(const fvb_device_spatial_wave_model &m)
    {
        return { { "SpatialArgs", m.spatial_args_size, sizeof(SpatialArgs) }, { "WaveLayout", m.wave_layout_size, spatial_wave_layout_size() },
            { "LDS doubles at FVB_MAX_PARAMS parameters", m.lds_probe, spatial_wave_model_lds_probe() } };
    }
    static const char *bad_params(const fvb_device_spatial_wave_model &)
    {
        return nullptr;
    }
    static std::string entry(const std::string &name, int)
    {
        return "wave-per-voxel spatial kernels of a device model named '" + name + "'";
    }
    static std::string absent(const std::string &name, int)
    {
        return "no " + entry(name, 0) + " are registered";
    }
};
// ... and the same two kernels in their form for 2 to FVB_MAX_PHIS noise precisions
// (include/fabber_device_spatial_wave_noise_model.h), by name: a registry of its own, an entry says which families its
// library compiled.
SpatialKernels get_spatial_kernels_wave_noise_model(int P, int N, bool need_f);
uint32_t spatial_wave_noise_model_lds_probe();
hipMemPool_t api_pool(); // (vb_api.hip: the engine's stream-ordered pool of the current device, or NULL)
template <> struct DeviceRegistryTraits<fvb_device_spatial_wave_noise_model>
{
    static constexpr const char *noun = "device spatial wave noise model", *is = "are";
    static constexpr int first_code = -24;
    static std::vector<DeviceStructSize> sizes(const fvb_device_spatial_wave_noise_model &m)
    {
        return { { "SpatialArgs", m.spatial_args_size, sizeof(SpatialArgs) }, { "WaveLayout", m.wave_layout_size, spatial_wave_layout_size() },
            { "LDS doubles at FVB_MAX_PARAMS parameters and FVB_MAX_PHIS precisions", m.lds_probe, spatial_wave_noise_model_lds_probe() } };
    }
    static const char *bad_params(const fvb_device_spatial_wave_noise_model &m)
    {
        return (m.families == 0 || (m.families & ~FVB_SPATIAL_WAVE_NOISE_PHIS) != 0)
            ? "the families mask does not name FVB_SPATIAL_WAVE_NOISE_PHIS, or names a family this engine does not know" : nullptr;
    }
    static std::string entry(const std::string &name, int)
    {
        return "wave-per-voxel noise-pattern spatial kernels of a device model named '" + name + "'";
    }
    static std::string absent(const std::string &name, int)
    {
        return "no " + entry(name, 0) + " are registered";
    }
};
// ... and the family's kernels under AR(1) noise with one echo (include/fabber_device_spatial_wave_ar_model.h), by name:
// a registry of its own (the reserved AR1 bit of the pattern registry above stays refused)
SpatialKernels get_spatial_kernels_wave_ar_model(int P, bool need_f);
uint32_t spatial_wave_ar_model_lds_probe();
template <> struct DeviceRegistryTraits<fvb_device_spatial_wave_ar_model>
{
    static constexpr const char *noun = "device spatial wave AR(1) model", *is = "are";
    static constexpr int first_code = -86, absent_code = -96; // (-90 is another registry's)
    static std::vector<DeviceStructSize> sizes(const fvb_device_spatial_wave_ar_model &m)
    {
        return { { "SpatialArgs", m.spatial_args_size, sizeof(SpatialArgs) }, { "WaveLayout", m.wave_layout_size, spatial_wave_layout_size() },
            { "LDS doubles under AR(1) noise at FVB_MAX_PARAMS parameters", m.lds_probe, spatial_wave_ar_model_lds_probe() } };
    }
    static const char *bad_params(const fvb_device_spatial_wave_ar_model &)
    {
        return nullptr;
    }
    static std::string entry(const std::string &name, int)
    {
        return "wave-per-voxel AR(1) spatial kernels of a device model named '" + name + "'";
    }
    static std::string absent(const std::string &name, int)
    {
        return "no " + entry(name, 0) + " are registered";
    }
};
} // namespace fvb
namespace
{

// What a configuration runs on: the kernel table, and for a body of a model library the launcher of its entry
struct SpatialRoute
{
    SpatialKernels k{};
    fvb_device_spatial_launch_fn library = nullptr;
    fvb_device_spatial_noise_launch_fn library_noise = nullptr; // ... of its entry for the noise policy `kind`
    int kind = FVB_SPNZ_WHITE;
    std::string name; // fabber_vb_spatial_kernel_name
    bool found() const
    {
        return k.setup != nullptr || library != nullptr || library_noise != nullptr;
    }
};
thread_local std::string g_spatial_kernel_name;
} // namespace

// A body of a model library: the table of the parameter count with the engine's own kernels wherever the model plays no
// part - the linear model's table serves, it covers 1 ... 8 parameters - and the three that evaluate the model left to
// the library's launcher. Under a noise pattern of 2 to 4 precisions and under AR(1) noise with one echo the same with the
// policy's table and the launcher of the library's entry for these policies (spatial_route_library_noise). Without a lane
// entry for (name, P) under white noise with one precision: the wave-per-voxel family around the body, where the library
// registered it (spatial_route_library_wave); without a lane entry that covers (name, P) under a noise pattern of 2 to 8
// precisions: the same family in its form for several precisions (spatial_route_library_wave_noise); without a lane entry
// for (name, P) under AR(1) noise with one echo: the family's AR(1) form (spatial_route_library_wave_ar). Nothing (-40) without an entry that covers the parameter count and the noise
// model, under the other noise models, or for a name without a wave body (which the argument checks answer with -16
// before this is asked).
static SpatialRoute spatial_route_library_noise(const fvb_config *cfg, int kind, const std::string &name)
{
    SpatialRoute route;
    fvb_device_spatial_noise_model entry;
    if ((kind != FVB_SPNZ_PATTERN2 && kind != FVB_SPNZ_PATTERN4 && kind != FVB_SPNZ_AR1)
        || !DeviceRegistry<fvb_device_spatial_noise_model>::instance().find(name, cfg->n_params, &entry))
        return route;
    const int family = kind == FVB_SPNZ_AR1 ? FVB_SPATIAL_NOISE_AR1 : FVB_SPATIAL_NOISE_PHIS;
    const int rows = kind == FVB_SPNZ_AR1 ? entry.state_rows_ar1 : (kind == FVB_SPNZ_PATTERN2 ? entry.state_rows_phis2 : entry.state_rows_phis4);
    if ((entry.families & family) == 0)
        return route;
    SpatialKernels k = get_spatial_kernels_nz_linear(cfg->n_params, cfg->need_f != 0, kind);
    if (!k.setup || k.wave || k.state_rows != rows) // (state_rows: compiled against another layout of the policy's statistics)
        return route;
    k.setup = k.noise = k.noise_fast = k.noise_acc = k.noise_fast_acc = nullptr; // the library's
    static const char *const tag[] = { "", "pattern2", "pattern4", "ar1" };
    route.name = "spatial<" + name + "," + std::to_string(cfg->n_params) + "," + tag[kind] + ">";
    k.name = nullptr; // (route.name)
    route.k = k;
    route.library_noise = entry.launch;
    route.kind = kind;
    return route;
}
// White noise with one precision and no lane entry for (name, P): the wave-per-voxel family where the library compiled its
// set-up kernel and second sweep around the body (include/fabber_device_spatial_wave_model.h), any parameter count the
// family takes. The engine's a_K kernels, first sweep and pack kernel of get_spatial_kernels_wide, the LDS of the layout
// with the body's parameter vectors; no split first sweep (prep, noise_fast are NULL: the run never asks for
// FVB_SPATIAL_KERNEL_NOISE_SPLIT).
static SpatialRoute spatial_route_library_wave(const fvb_config *cfg, const std::string &name)
{
    SpatialRoute route;
    fvb_device_spatial_wave_model entry;
    if (cfg->n_params < 1 || cfg->n_params > FVB_MAX_PARAMS || !DeviceRegistry<fvb_device_spatial_wave_model>::instance().find(name, 0, &entry))
        return route;
    const SpatialKernels k = get_spatial_kernels_wave_model(cfg->n_params, cfg->need_f != 0);
    if (!k.theta || !k.wave)
        return route;
    route.name = "spatial<" + name + ",wave>";
    route.k = k;
    route.library = entry.launch;
    return route;
}
// A noise pattern and no lane entry for (name, P) that covers it: the wave-per-voxel family in its form for N = n_phis
// classes where the library compiled it (include/fabber_device_spatial_wave_noise_model.h). The engine's a_K kernels and
// pack kernel, its first sweep for N classes, the state image with the class rows, the LDS of the layout for (P, N).
static SpatialRoute spatial_route_library_wave_noise(const fvb_config *cfg, int kind, const std::string &name)
{
    SpatialRoute route;
    fvb_device_spatial_wave_noise_model entry;
    if ((kind != FVB_SPNZ_PATTERN2 && kind != FVB_SPNZ_PATTERN4 && kind != FVB_SPNZ_PATTERN8) || cfg->n_params < 1
        || cfg->n_params > FVB_MAX_PARAMS || !DeviceRegistry<fvb_device_spatial_wave_noise_model>::instance().find(name, 0, &entry)
        || (entry.families & FVB_SPATIAL_WAVE_NOISE_PHIS) == 0)
        return route;
    const SpatialKernels k = get_spatial_kernels_wave_noise_model(cfg->n_params, cfg->n_phis, cfg->need_f != 0);
    if (!k.theta || !k.wave)
        return route;
    route.name = "spatial<" + name + ",wave,phis" + std::to_string(cfg->n_phis) + ">";
    route.k = k;
    route.library = entry.launch;
    return route;
}
// AR(1) noise with one echo and no lane entry for (name, P) with the AR1 family: the wave-per-voxel family in its AR(1) form
// where the library compiled it (include/fabber_device_spatial_wave_ar_model.h). The engine's a_K kernels and pack kernel,
// its first sweep (with the AR free energy where F is evaluated), the state image with the rows of SpAr1, the LDS of the
// layout with the AR areas.
static SpatialRoute spatial_route_library_wave_ar(const fvb_config *cfg, int kind, const std::string &name)
{
    SpatialRoute route;
    fvb_device_spatial_wave_ar_model entry;
    if (kind != FVB_SPNZ_AR1 || cfg->n_params < 1 || cfg->n_params > FVB_MAX_PARAMS
        || !DeviceRegistry<fvb_device_spatial_wave_ar_model>::instance().find(name, 0, &entry))
        return route;
    const SpatialKernels k = get_spatial_kernels_wave_ar_model(cfg->n_params, cfg->need_f != 0);
    if (!k.theta || !k.wave)
        return route;
    route.name = "spatial<" + name + ",wave,ar1>";
    route.k = k;
    route.library = entry.launch;
    return route;
}
static SpatialRoute spatial_route_library(const fvb_config *cfg, int kind)
{
    SpatialRoute route;
    const std::string name = config_device_model(cfg);
    fvb_device_spatial_model entry;
    if (cfg->params_ext || name.empty() || !find_wave_body(name))
        return route;
    if (kind != FVB_SPNZ_WHITE)
    {
        route = spatial_route_library_noise(cfg, kind, name);
        if (route.found())
            return route;
        return kind == FVB_SPNZ_AR1 ? spatial_route_library_wave_ar(cfg, kind, name) : spatial_route_library_wave_noise(cfg, kind, name);
    }
    if (!DeviceRegistry<fvb_device_spatial_model>::instance().find(name, cfg->n_params, &entry))
        return spatial_route_library_wave(cfg, name);
    SpatialKernels k = get_spatial_kernels_linear(cfg->n_params, cfg->need_f != 0);
    if (!k.setup || k.wave || k.lds_classes || k.state_rows != entry.state_rows) // (state_rows: compiled against another SpLayout)
        return route;
    k.setup = k.noise = k.noise_fast = k.noise_acc = k.noise_fast_acc = nullptr; // the library's
    route.name = "spatial<" + name + "," + std::to_string(cfg->n_params) + ">";
    k.name = nullptr; // (route.name)
    route.k = k;
    route.library = entry.launch;
    return route;
}

// the kernel table of a configuration (none: no kernels were built for this model / parameter count / noise model)
static SpatialKernels spatial_kernels_builtin(const fvb_config *cfg, int kind)
{
    const int P = cfg->n_params;
    const bool need_f = cfg->need_f != 0;
    if (kind >= FVB_SPNZ_ARN2 && kind <= FVB_SPNZ_ARN4)
        return get_spatial_kernels_nz_arn(cfg->model, P, need_f, kind);
    if (kind == FVB_SPNZ_PATTERN8)
        return get_spatial_kernels_nz_pattern8(cfg->model, P, need_f);
    switch (cfg->model)
    {
    case FVB_MODEL_POLY:
        return kind == FVB_SPNZ_WHITE ? get_spatial_kernels_poly(P, need_f) : get_spatial_kernels_nz_poly(P, need_f, kind);
    case FVB_MODEL_LINEAR:
        return kind == FVB_SPNZ_WHITE ? get_spatial_kernels_linear(P, need_f) : get_spatial_kernels_nz_linear(P, need_f, kind);
    case FVB_MODEL_EXP:
        return kind == FVB_SPNZ_WHITE ? get_spatial_kernels_exp(P, need_f) : get_spatial_kernels_nz_exp(P, need_f, kind);
    case FVB_MODEL_HOSTJAC:
        return kind == FVB_SPNZ_WHITE ? get_spatial_kernels_host(P, need_f) : get_spatial_kernels_nz_host(P, need_f, kind);
    default:
        return SpatialKernels{};
    }
}
static SpatialRoute spatial_kernels_for(const fvb_config *cfg)
{
    const int kind = spatial_noise_kind(cfg);
    if (kind < 0)
        return SpatialRoute{};
    if (cfg->model == FVB_MODEL_PLUGIN)
        return spatial_route_library(cfg, kind);
    SpatialRoute route;
    route.k = spatial_kernels_builtin(cfg, kind);
    if (route.k.setup && route.k.name)
        route.name = route.k.name;
    return route;
}
// what a configuration without a kernel table (-40) is told
static const char *const spatial_init_mvn_refusal
    = "a device model of a library needs the initial posterior as init_mvn (the model's InitVoxelPosterior runs on the host)";
static std::string spatial_kernels_refusal(const fvb_config *cfg)
{
    if (cfg->model == FVB_MODEL_HOSTJAC && cfg->n_params > 8 && spatial_noise_kind(cfg) != FVB_SPNZ_WHITE)
        return "spatial VB with more than 8 parameters runs white noise with one noise precision (noise patterns and AR(1) "
               "noise: up to 6 parameters of a model evaluated on the host)";
    return "no spatial kernel instantiation for this model / parameter count / noise model";
}

// What the steps of open() hand on: the geometry the device worked out, the plan, and the host arrays whose uploads
// are in flight until publish_args() has waited for the stream.
struct fvb_spatial_run::Geometry
{
    DevMem d_coords; // the co-ordinates on the device (kept from the neighbour table's kernels; empty: host table)
    GeomScan scan;
    plan::PriorScan priors;
    plan::SlabParams slab;
    plan::SlabNumbering numbering; // (slab form)
    int n_pos = 0, sl_width = 64;
    std::vector<int32_t> order = std::vector<int32_t>(1), seg_start; // (per-level form: the level order)
    double aK0[FVB_MAX_PARAMS];
};

int fvb_spatial_run::open(const fvb_config *cfg_, const fvb_spatial *sp_, const void *d_data, const fvb_outputs *d_out,
    hipStream_t stream_)
{
    env = SpatialEnv::read();
    cfg = *cfg_;
    sp = *sp_;
    stream = stream_;
    V = cfg.n_voxels;
    P = cfg.n_params;
    owned_begin = 0;
    owned_end = V;
    if (sp.owned_end > sp.owned_begin)
    {
        owned_begin = sp.owned_begin;
        owned_end = sp.owned_end;
    }
    if (owned_begin < 0 || owned_end > V)
        return api_fail(-45, "owned voxel range outside the local voxel list");
    if (spatial_noise_kind(&cfg) < 0)
        return api_fail(-44, spatial_noise_refusal);
    {
        const SpatialRoute route = spatial_kernels_for(&cfg);
        if (!route.found())
            return api_fail(-40, spatial_kernels_refusal(&cfg));
        k = route.k;
        library = route.library;
        library_noise = route.library_noise;
        library_kind = route.kind;
    }
    if ((library || library_noise) && !cfg.init_mvn)
    {
        // the library's initial-posterior kernel (include/fabber_device_init_model.h) writes the image for every local
        // voxel, on this run's stream: the set-up kernel's stream waits for that stream before it starts (start_setup)
        fvb_device_init_model init_entry;
        if (!find_init_entry(&cfg, &init_entry))
            return api_fail(-52, spatial_init_mvn_refusal);
        if (V > 0)
        {
            FVB_HIP_CHECK(d_init_mvn.alloc(sizeof(double) * (size_t)fabber_vb_mvn_rows(P + noise_outputs(&cfg)) * (size_t)V, stream));
            const int rc_init = launch_init_entry(init_entry, &cfg, d_data, (double *)d_init_mvn.p, stream);
            if (rc_init)
                return rc_init;
            cfg.init_mvn = (const double *)d_init_mvn.p;
        }
    }
    if (cfg.model == FVB_MODEL_HOSTJAC && !lin_next) // (the kernels read the host's linearisations)
        return api_fail(-56, "a model evaluated on the host runs spatial VB through fabber_vb_run_spatial_hostmodel_host");
    noise_lds = k.lds_classes ? (size_t)cfg.n_times : 0;

    auto ms_since = [](std::chrono::steady_clock::time_point a) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    };
    int rc;
    Geometry g;
    if ((rc = start_setup(d_data, d_out)) != 0)
        return rc;
    const auto t_start = std::chrono::steady_clock::now();
    if ((rc = neighbour_table(g)) != 0)
        return rc;
    t_neighbours_ms = ms_since(t_start);
    if ((rc = plan_sweeps(g)) != 0)
        return rc;
    t_geometry_ms = ms_since(t_start);
    if ((rc = upload_plan(g)) != 0)
        return rc;
    return publish_args();
}

// Vb::SetupPerVoxelDists for every local voxel (ghosts included: their initial means are what the neighbouring slab
// starts from too) needs the series and the options only: it runs on a stream of its own while the host and this
// run's stream work out the geometry. `sa` gets the fields that need no geometry here - what the set-up kernel is
// launched with; upload_plan() adds the rest.
int fvb_spatial_run::start_setup(const void *d_data, const fvb_outputs *d_out)
{
    const bool wave_ar = k.wave && cfg.noise == FVB_NOISE_AR1;
    if (k.wave && (cfg.n_phis > 1 || wave_ar))
    {
        // the state image with every class's statistics (46 KB per voxel at 32 parameters and 8 precisions) or with the
        // AR(1) moments (19 KB per voxel at 32 parameters): worked out before the run, a device that cannot hold it says
        // so instead of failing inside the allocation
        const size_t bytes = sizeof(double) * (size_t)k.state_rows * (size_t)V;
        size_t free_bytes = 0, total_bytes = 0;
        FVB_HIP_CHECK(hipMemGetInfo(&free_bytes, &total_bytes));
        // (what the engine's pool keeps from earlier runs is not free to the driver, but it is to this allocation)
        uint64_t reserved = 0, used = 0;
        if (hipMemPool_t pool = fvb::api_pool())
            if (hipMemPoolGetAttribute(pool, hipMemPoolAttrReservedMemCurrent, &reserved) == hipSuccess
                && hipMemPoolGetAttribute(pool, hipMemPoolAttrUsedMemCurrent, &used) == hipSuccess && reserved > used)
                free_bytes += (size_t)(reserved - used);
        (void)hipGetLastError();
        if (bytes > free_bytes)
            return api_fail(-40, "spatial VB with " + std::to_string(P) + " parameters and "
                    + (wave_ar ? std::string("AR(1) noise") : std::to_string(cfg.n_phis) + " noise precisions") + " keeps " + std::to_string(k.state_rows) + " rows per voxel: " + std::to_string(bytes >> 20) + " MiB for "
                    + std::to_string(V) + " voxels, the device has " + std::to_string(free_bytes >> 20) + " MiB free");
        if (k.wave_lds > 64 * 1024) // (more dynamic LDS than a kernel gets without asking; the library's launcher asks for its own)
            FVB_HIP_CHECK(hipFuncSetAttribute((const void *)k.theta, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.wave_lds));
    }
    FVB_HIP_CHECK(d_state.alloc(sizeof(double) * (size_t)k.state_rows * V, stream));
    FVB_HIP_CHECK(d_status.alloc(sizeof(int32_t) * (size_t)V, stream));
    memset(&sa, 0, sizeof(sa));
    sa.ka.n_unmasked = cfg.n_times;
    sa.nz_count[0] = (double)cfg.n_times; // timepoints per noise precision (trace of Q_k)
    if (cfg.phi_index) // (a device pointer here: read it back once)
    {
        std::vector<uint8_t> h(cfg.n_times);
        FVB_HIP_CHECK(hipMemcpyAsync(h.data(), cfg.phi_index, h.size(), hipMemcpyDeviceToHost, stream));
        FVB_HIP_CHECK(hipStreamSynchronize(stream));
        sa.ka.n_unmasked = 0;
        sa.nz_count[0] = 0;
        for (int t = 0; t < cfg.n_times; t++)
        {
            sa.ka.n_unmasked += (h[t] != 255);
            if (h[t] < 8)
                sa.nz_count[h[t]] += 1;
        }
    }
    sa.lin_cur = lin_cur;
    sa.lin_next = lin_next;
    sa.ka.cfg = cfg;
    sa.ka.out = *d_out;
    sa.ka.data = d_data;
    sa.ka.residual_mode = api_residual_mode();
    sa.ka.residual_tol = api_residual_tol();
    sa.ka.precise_passes = api_precise_passes();
    sa.state = (double *)d_state.p;
    sa.status = (int32_t *)d_status.p;
    sa.owned_begin = owned_begin;
    sa.owned_end = owned_end;
    sa.locked_centres = sp.locked_centres;
    sa.locked_linear = sp.locked_centres != nullptr;
    FVB_HIP_CHECK(fvb::api_take_side_stream(&setup_stream, &setup_device));
    FVB_HIP_CHECK(hipEventCreateWithFlags(&setup_done, hipEventDisableTiming));
    // (the two buffers were allocated in `stream`'s order; the series is the caller's, complete in `stream`'s order too)
    FVB_HIP_CHECK(hipEventRecord(setup_done, stream));
    FVB_HIP_CHECK(hipStreamWaitEvent(setup_stream, setup_done, 0));
    // (the wave-per-voxel family: one workgroup per voxel)
    const int rc = launch_model_kernel(FVB_SPATIAL_KERNEL_SETUP, k.setup, (unsigned)(k.wave ? V : (V + 63) / 64),
        k.wave ? k.wave_lds : noise_lds, setup_stream);
    if (rc)
        return rc;
    FVB_HIP_CHECK(hipEventRecord(setup_done, setup_stream));
    return 0;
}

// The three launches of a run that evaluate the model - set-up, the second sweep and the second sweep of the split form -
// with the run's arguments `sa` by value: the engine's own kernel, or the launcher of a model library for the kernels
// in its code object (64-lane workgroups either way)
int fvb_spatial_run::launch_model_kernel(int which, SpatialKernelFn fn, unsigned grid, size_t lds, hipStream_t on)
{
    if (library || library_noise)
    {
        char err[256] = "";
        const int rc = library_noise ? library_noise(library_kind, which, cfg.need_f != 0, &sa, grid, (uint32_t)lds, on, err, (int32_t)sizeof(err))
                                     : library(which, cfg.need_f != 0, &sa, grid, (uint32_t)lds, on, err, (int32_t)sizeof(err));
        return rc ? api_fail(rc, err[0] ? err : "the launcher of a device model's spatial kernels failed") : 0;
    }
    hipLaunchKernelGGL(fn, dim3(grid), dim3(64), lds, on, sa);
    FVB_HIP_CHECK(hipGetLastError());
    return 0;
}

// the neighbour table: on the device where the geometry allows, else on the host
int fvb_spatial_run::neighbour_table(Geometry &g)
{
    FVB_HIP_CHECK(d_nn.alloc(sizeof(int32_t) * (size_t)V * 6, stream));
    FVB_HIP_CHECK(d_nn_dir.alloc(sizeof(int32_t) * (size_t)std::max(V, 1), stream));
    std::string err;
    const int on_device = (V > 0 && !env.host_geometry)
        ? build_neighbours_device(sp.coords, V, sp.spatial_dims, (int32_t *)d_nn.p, (int32_t *)d_nn_dir.p, stream, err, &g.d_coords, &g.scan, &dense) : 1;
    if (on_device < 0)
        return api_fail(on_device, err);
    if (on_device == 1)
    {
        std::vector<int32_t> nn, dirs;
        err = plan::build_neighbours(sp.coords, V, sp.spatial_dims, nn, &dirs);
        if (!err.empty())
            return api_fail(-41, err);
        FVB_HIP_CHECK(hipMemcpyAsync(d_nn.p, nn.data(), sizeof(int32_t) * (size_t)V * 6, hipMemcpyHostToDevice, stream));
        FVB_HIP_CHECK(hipMemcpyAsync(d_nn_dir.p, dirs.data(), sizeof(int32_t) * (size_t)V, hipMemcpyHostToDevice, stream));
        FVB_HIP_CHECK(hipStreamSynchronize(stream)); // nn is a local
    }
    return 0;
}

// The form of the first sweep and its order: the slab-major numbering of the split sweep where the run is eligible
// and the kernel takes it (the slab form numbers the voxels itself and does without the level order - 2.5 ms of a
// 128^3 run's set-up), else the level order the per-level launches walk.
int fvb_spatial_run::plan_sweeps(Geometry &g)
{
    const plan::Owned own(sp.coords, V, owned_begin, owned_end);
    g.priors = plan::scan_priors(P, cfg.prior_type, cfg.prior_prec, cfg.prior_mean);
    has_spatial |= g.priors.has_spatial;
    const plan::HostThreads th(own.n(), env.host_threads);
    plan::Levels lv = plan::scan_levels(own, 1, 1, th);
    const bool eligible = allow_fast && k.prep && has_spatial && !g.priors.minus_zero && (own.whole() || multi_fast) && own.n() > 0
        && !env.per_level;
    slab_form = false;
    if (eligible && lv.range() < plan::MAX_LEVEL_RANGE)
    {
        int cus = 256, dev_now = 0;
        if (hipGetDevice(&dev_now) == hipSuccess)
            (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev_now);
        const long long cap = plan::slab_cap(cus, device_share);
        // (with the co-ordinates on the device - the usual case - the numbering is three small kernels there; the
        // host does it with its threads otherwise: 3 ms at 128^3 against 0.2)
        // (a slab with ghost planes is numbered on the host: the device kernels number every local voxel)
        if (g.d_coords.p != nullptr && !env.host_numbering && own.whole())
        {
            const int rc = number_slabs_device(g, lv, cap);
            if (rc)
                return rc;
        }
        else
            slab_form = plan::number_slabs(own, lv, cap, env.slab_dz, sp.spatial_dims, th, g.slab, g.numbering);
        if (slab_form)
        {
            g.n_pos = (own.n() + 15) / 16 * 16;
            g.sl_width = plan::slab_width(g.numbering.sl_max_run, env.slab_width);
            level_begin_counts = g.numbering.level_count;
        }
    }
    if (!slab_form)
    {
        // the per-level launches: the exact form, with the second-neighbour levels where types P, p are about
        if (g.priors.second_neighbours)
            lv = plan::scan_levels(own, 2, 3, th);
        plan::LevelOrder lo = plan::build_level_order(own, lv, th);
        level_begin = std::move(lo.level_begin);
        level_value = std::move(lo.level_value);
        g.order = std::move(lo.order);
        std::copy(lo.level_w, lo.level_w + 3, level_w);
    }
    fast = slab_form;
    if (slab_form && !own.whole())
        plan::mark_ghosts(own, g.numbering.pos_of);
    if (multi_fast)
        h_pos_of = g.numbering.pos_of;
    return 0;
}

// the slab-major numbering with the co-ordinates on the device: a histogram over the keys, plan::slab_prefix on the
// host (a few ten thousand keys) and one more pass that hands out the positions of a key's run (d_pos_of)
int fvb_spatial_run::number_slabs_device(Geometry &g, const plan::Levels &lv, long long slab_cap)
{
    g.slab = plan::slab_params(g.scan.zmin, g.scan.zmax, lv, slab_cap, env.slab_dz);
    const plan::SlabParams &p = g.slab;
    if (!p.usable(sp.spatial_dims))
        return 0;
    const size_t nk = p.n_keys();
    std::vector<std::vector<int32_t> > count(1, std::vector<int32_t>(nk, 0));
    DevMem d_keys;
    const unsigned vgrid = (unsigned)((V + 255) / 256);
    FVB_HIP_CHECK(d_keys.alloc(sizeof(int32_t) * nk, stream));
    FVB_HIP_CHECK(hipMemsetAsync(d_keys.p, 0, sizeof(int32_t) * nk, stream));
    hipLaunchKernelGGL(slab_count_kernel, dim3(vgrid), dim3(256), 0, stream, (const int32_t *)g.d_coords.p, V, p.zmin, (int)p.dz,
        (int)p.lmin, (int)p.nl, (int32_t *)d_keys.p);
    FVB_HIP_CHECK(hipMemcpyAsync(count[0].data(), d_keys.p, sizeof(int32_t) * nk, hipMemcpyDeviceToHost, stream));
    FVB_HIP_CHECK(hipStreamSynchronize(stream));
    g.numbering = plan::slab_prefix(count, p);
    if (!plan::slab_accepted(g.numbering, p, slab_cap))
    {
        g.numbering = plan::SlabNumbering();
        return 0;
    }
    // count[0] holds every key's first position now: hand the positions out on the device
    FVB_HIP_CHECK(d_pos_of.alloc(sizeof(int32_t) * (size_t)V, stream));
    FVB_HIP_CHECK(hipMemcpyAsync(d_keys.p, count[0].data(), sizeof(int32_t) * nk, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(slab_place_kernel, dim3(vgrid), dim3(256), 0, stream, (const int32_t *)g.d_coords.p, V, p.zmin, (int)p.dz,
        (int)p.lmin, (int)p.nl, (int32_t *)d_keys.p, (int32_t *)d_pos_of.p);
    FVB_HIP_CHECK(hipGetLastError());
    FVB_HIP_CHECK(hipStreamSynchronize(stream)); // (count[0] and d_keys go out of scope)
    slab_form = true;
    return 0;
}

// device memory of the run and the rest of `sa`
int fvb_spatial_run::upload_plan(Geometry &g)
{
    g.seg_start = plan::ak_segments(plan::Owned(sp.coords, V, owned_begin, owned_end));
    const int n_blocks = (int)g.seg_start.size() - 1;
    n_segments = n_blocks;
    FVB_HIP_CHECK(d_order.alloc(sizeof(int32_t) * g.order.size(), stream));
    FVB_HIP_CHECK(d_aK.alloc(sizeof(double) * FVB_MAX_PARAMS, stream));
    FVB_HIP_CHECK(d_sums.alloc(sizeof(double) * FVB_MAX_PARAMS * 2, stream));
    FVB_HIP_CHECK(d_partials.alloc(sizeof(double) * (size_t)std::max(n_blocks, 1) * P * 2, stream));
    FVB_HIP_CHECK(d_seg_start.alloc(sizeof(int32_t) * g.seg_start.size(), stream));
    FVB_HIP_CHECK(hipMemcpyAsync(d_seg_start.p, g.seg_start.data(), sizeof(int32_t) * g.seg_start.size(), hipMemcpyHostToDevice, stream));
    FVB_HIP_CHECK(d_fprior.alloc(sizeof(double), stream));
    FVB_HIP_CHECK(hipMemcpyAsync(d_order.p, g.order.data(), sizeof(int32_t) * g.order.size(), hipMemcpyHostToDevice, stream));
    for (int i = 0; i < FVB_MAX_PARAMS; i++)
        g.aK0[i] = 1e-8; // priors.cc:185
    FVB_HIP_CHECK(hipMemcpyAsync(d_aK.p, g.aK0, sizeof(g.aK0), hipMemcpyHostToDevice, stream));
    FVB_HIP_CHECK(hipMemsetAsync(d_fprior.p, 0, sizeof(double), stream));
    FVB_HIP_CHECK(hipMemsetAsync(d_sums.p, 0, sizeof(double) * FVB_MAX_PARAMS * 2, stream));
    FVB_HIP_CHECK(hipMemsetAsync(d_partials.p, 0, sizeof(double) * (size_t)std::max(n_blocks, 1) * P * 2, stream));

    sa.nn = (const int32_t *)d_nn.p;
    sa.nn_dir = (const int32_t *)d_nn_dir.p;
    sa.order = (const int32_t *)d_order.p;
    sa.aK = (double *)d_aK.p;
    sa.ak_sums = (double *)d_sums.p;
    sa.partials = (double *)d_partials.p;
    sa.seg_start = (const int32_t *)d_seg_start.p;
    sa.fprior_last = (double *)d_fprior.p;
    sa.spatial_dims = sp.spatial_dims;
    sa.update_first_iter = sp.update_first_iter;
    sa.spatial_speed = sp.spatial_speed;
    sa.q1 = sp.q1;
    sa.q2 = sp.q2;
    sa.n_blocks = n_blocks;
    sa.n_voxels_global = sp.n_voxels_global > 0 ? sp.n_voxels_global : V;
    return fast ? upload_slab_form(g) : 0;
}

// ... of the slab form of the split sweep: the numbering, the records, the inboxes, the prep kernel's tiles
int fvb_spatial_run::upload_slab_form(const Geometry &g)
{
    const plan::SlabNumbering &nb = g.numbering;
    const size_t NP = (size_t)g.n_pos, ns = (size_t)g.priors.n_spatial;
    if (!d_pos_of.p)
    {
        FVB_HIP_CHECK(d_pos_of.alloc(sizeof(int32_t) * (size_t)V, stream));
        FVB_HIP_CHECK(hipMemcpyAsync(d_pos_of.p, nb.pos_of.data(), sizeof(int32_t) * (size_t)V, hipMemcpyHostToDevice, stream));
    }
    FVB_HIP_CHECK(d_level_pos.alloc(sizeof(int32_t) * nb.level_pos.size(), stream));
    FVB_HIP_CHECK(d_level_count.alloc(sizeof(int32_t) * nb.level_count.size(), stream));
    FVB_HIP_CHECK(hipMemcpyAsync(d_level_pos.p, nb.level_pos.data(), sizeof(int32_t) * nb.level_pos.size(), hipMemcpyHostToDevice, stream));
    FVB_HIP_CHECK(hipMemcpyAsync(d_level_count.p, nb.level_count.data(), sizeof(int32_t) * nb.level_count.size(), hipMemcpyHostToDevice, stream));
    // doubles: x, pm, pre, rhsk, pprec, q [ns][NP] each; sigk [ns][ns][NP]; nbr [ns][3][NP]
    const size_t n_f64 = std::max<size_t>(1, (6 * ns + ns * ns + 3 * ns) * NP);
    FVB_HIP_CHECK(d_sw_f64.alloc(sizeof(double) * n_f64, stream));
    const size_t n_i32 = 5 * NP;
    FVB_HIP_CHECK(d_sw_i32.alloc(sizeof(int32_t) * n_i32, stream)); // npos [4][NP], alive [NP]
    FVB_HIP_CHECK(d_sw_sync.alloc(64, stream));                      // flags
    const size_t gran_bytes = std::max<size_t>(16, sizeof(unsigned long long) * 2 * ns * NP);
    if (multi_fast)
    {
        FVB_HIP_CHECK(d_sw_gran.alloc_fine(gran_bytes));
        gran_fine = d_sw_gran.fine;
    }
    else
        FVB_HIP_CHECK(d_sw_gran.alloc(gran_bytes, stream));
    FVB_HIP_CHECK(hipMemsetAsync(d_sw_gran.p, 0, gran_bytes, stream));
    sa.sl_remote = multi_fast ? 1 : 0;
    sa.sw_gran = (unsigned long long *)d_sw_gran.p;
    sa.sw_serial = 0;
    FVB_HIP_CHECK(hipMemsetAsync(d_sw_i32.p, 0, sizeof(int32_t) * n_i32, stream));
    FVB_HIP_CHECK(hipMemsetAsync(d_sw_f64.p, 0, sizeof(double) * n_f64, stream));
    FVB_HIP_CHECK(hipMemsetAsync(d_sw_sync.p, 0, 64, stream));
    double *f = (double *)d_sw_f64.p;
    sa.sw_x = f;
    sa.sw_pm = f + ns * NP;
    sa.sw_pre = f + 2 * ns * NP;
    sa.sw_rhsk = f + 3 * ns * NP;
    sa.sw_pprec = f + 4 * ns * NP;
    sa.sw_q = f + 5 * ns * NP;
    sa.sw_sigk = f + 6 * ns * NP;
    sa.sw_nbr = f + (6 * ns + ns * ns) * NP;
    FVB_HIP_CHECK(d_slab_first.alloc(sizeof(int32_t) * nb.slab_first.size(), stream));
    FVB_HIP_CHECK(hipMemcpyAsync(d_slab_first.p, nb.slab_first.data(), sizeof(int32_t) * nb.slab_first.size(), hipMemcpyHostToDevice, stream));
    sa.n_slabs = (int32_t)nb.slab_first.size() - 1;
    sa.sl_first_run = (const int32_t *)d_slab_first.p;
    sa.sl_width = g.sl_width;
    sa.sl_max_run = nb.sl_max_run;
    max_runs_per_slab = plan::max_runs_per_slab(nb.slab_first);
    sa.sw_npos = (int32_t *)d_sw_i32.p;
    sa.sw_alive = (int32_t *)d_sw_i32.p + 4 * NP;
    sa.sw_flags = (int32_t *)d_sw_sync.p + 4;
    sa.pos_of = (const int32_t *)d_pos_of.p;
    sa.n_pos = g.n_pos;
    sa.n_spatial = g.priors.n_spatial;
    for (int i = 0; i < g.priors.n_spatial; i++)
        sa.spatial_param[i] = g.priors.spatial_param[i];
    sa.sw_level_pos = (const int32_t *)d_level_pos.p;
    sa.sw_level_count = (const int32_t *)d_level_count.p;
    sa.n_levels = (int32_t)nb.level_pos.size();
    if (dense.map.p && !env.prep_linear) // the prep kernel's tiles (vb_spatial.h)
    {
        const int32_t *Z = sp.coords + 2 * (size_t)V;
        const plan::PrepTiles t = plan::prep_tiles(dense.xsize, dense.ysize, Z[owned_begin], Z[owned_end - 1], owned_end - owned_begin);
        if (t.n_tiles > 0)
        {
            sa.dense = (const int32_t *)dense.map.p;
            sa.dense_base = dense.base;
            sa.dense_span = dense.span;
            sa.xsize = dense.xsize;
            sa.ysize = dense.ysize;
            sa.tile_nx = t.tile_nx;
            sa.tile_ny = t.tile_ny;
            sa.tile_z0 = t.tile_z0;
            sa.n_tiles = t.n_tiles;
        }
    }
    return 0;
}

// the argument block the per-level launches read (nothing in it changes per launch), on the device
int fvb_spatial_run::publish_args()
{
    FVB_HIP_CHECK(d_sa.alloc(sizeof(SpatialArgs), stream));
    FVB_HIP_CHECK(hipMemcpyAsync(d_sa.p, &sa, sizeof(SpatialArgs), hipMemcpyHostToDevice, stream));
    FVB_HIP_CHECK(hipStreamSynchronize(stream)); // `sa`, the plan's arrays are pageable host memory

    // everything after this waits for the set-up kernel (started at the top)
    FVB_HIP_CHECK(hipStreamWaitEvent(stream, setup_done, 0));
    return 0;
}

int fvb_spatial_run::ak_sums(double *host_sums)
{
    hipLaunchKernelGGL(k.ak_partial, dim3(sa.n_blocks), dim3(256), 0, stream, sa);
    hipLaunchKernelGGL(k.ak_reduce, dim3(1), dim3(64), 0, stream, sa);
    FVB_HIP_CHECK(hipGetLastError());
    if (host_sums)
    {
        FVB_HIP_CHECK(hipMemcpyAsync(host_sums, d_sums.p, sizeof(double) * 2 * P, hipMemcpyDeviceToHost, stream));
        FVB_HIP_CHECK(hipStreamSynchronize(stream));
    }
    return 0;
}

// the segments' partial sums [n_segments][P][2] (for callers that add up several slabs' segments in order)
int fvb_spatial_run::ak_segment_sums(double *host_partials)
{
    if (sa.n_blocks > 0)
        hipLaunchKernelGGL(k.ak_partial, dim3(sa.n_blocks), dim3(256), 0, stream, sa);
    FVB_HIP_CHECK(hipGetLastError());
    FVB_HIP_CHECK(hipMemcpyAsync(host_partials, d_partials.p, sizeof(double) * 2 * P * (size_t)sa.n_blocks, hipMemcpyDeviceToHost, stream));
    FVB_HIP_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int fvb_spatial_run::set_ak_sums(const double *host_sums)
{
    if (host_sums)
        FVB_HIP_CHECK(hipMemcpyAsync(d_sums.p, host_sums, sizeof(double) * 2 * P, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k.ak_final, dim3(1), dim3(64), 0, stream, sa);
    FVB_HIP_CHECK(hipGetLastError());
    if (host_sums)
        FVB_HIP_CHECK(hipStreamSynchronize(stream)); // the caller's buffer is pageable
    return 0;
}

int fvb_spatial_run::sweep(int it)
{
    int rc = sweep_levels(it, LLONG_MIN, LLONG_MAX);
    return rc ? rc : sweep_noise(it);
}

// first sweep, the levels with lo <= value < hi (one launch per level)
int fvb_spatial_run::sweep_levels(int it, long long lo, long long hi)
{
    sa.it = it;
    const SpatialArgs *sap = (const SpatialArgs *)d_sa.p;
    for (size_t l = 0; l + 1 < level_begin.size(); l++)
    {
        if (level_value[l] < lo || level_value[l] >= hi)
            continue;
        const int begin = level_begin[l], count = level_begin[l + 1] - level_begin[l];
        hipLaunchKernelGGL(k.theta, dim3((unsigned)(k.wave ? count : (count + 63) / 64)), dim3(64), k.wave ? k.wave_lds : 0, stream,
            sap, begin, count, it);
    }
    FVB_HIP_CHECK(hipGetLastError());
    return 0;
}

int fvb_spatial_run::sweep_noise(int it)
{
    sa.it = it;
    const int n_owned = owned_end - owned_begin;
    if (n_owned > 0)
        return launch_model_kernel(FVB_SPATIAL_KERNEL_NOISE, second_sweep(false, it), (unsigned)(k.wave ? n_owned : (n_owned + 63) / 64),
            k.wave ? k.wave_lds : noise_lds, stream);
    return 0;
}

// One iteration's first and second sweep with the split first sweep (see vb_spatial.h)
// the three launches of an iteration with the slab form of the split sweep, one by one (a run of several slabs on several
// devices puts its exchanges between them; one device runs them back to back: sweep_fast)
int fvb_spatial_run::fast_prep(int it)
{
    sa.it = it;
    sa.sw_serial++; // this sweep's number
    const int n_owned = owned_end - owned_begin;
    // (a multiple of 8 workgroups: the kernel deals them out to the XCDs in contiguous eighths of the voxel list)
    const int waves = sa.n_tiles > 0 ? sa.n_tiles : (n_owned + 63) / 64;
    hipLaunchKernelGGL(k.prep, dim3((unsigned)((waves + 7) / 8 * 8)), dim3(64), 0, stream, (const SpatialArgs *)d_sa.p, it, sa.sw_serial);
    FVB_HIP_CHECK(hipGetLastError());
    return 0;
}
int fvb_spatial_run::fast_sweep()
{
    if (sa.n_spatial == 0) // (types P, p only: nothing waits for a neighbour)
        return 0;
    const int which = sa.n_spatial <= 1 ? 0 : (sa.n_spatial == 2 ? 1 : 2);
    // one workgroup of 1024 lanes per slab (within the device's compute units, see the numbering)
    if (sa.n_spatial > 8)
        return api_fail(-40, "more than eight parameters with a first-neighbour prior");
    const size_t lds = sizeof(double) * (8 + 2 * (size_t)sa.n_spatial * sa.sl_max_run) + sizeof(int32_t) * (2 * (size_t)max_runs_per_slab + 2);
    if (lds > 48 * 1024)
        FVB_HIP_CHECK(hipFuncSetAttribute((const void *)k.slab_sweep[which], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k.slab_sweep[which], dim3((unsigned)sa.n_slabs), dim3(1024), lds, stream, sa);
    FVB_HIP_CHECK(hipGetLastError());
    return 0;
}
int fvb_spatial_run::fast_noise(int it)
{
    sa.it = it;
    const int n_owned = owned_end - owned_begin;
    return launch_model_kernel(FVB_SPATIAL_KERNEL_NOISE_SPLIT, second_sweep(true, it), (unsigned)((n_owned + 63) / 64), noise_lds, stream);
}

// This slab's top plane hands its new means to the bottom plane of `upper` (another device, or another stream of this
// one): where in upper's granule array the inbox of every top-plane voxel's z+1 neighbour is. global_first = the global
// index of this slab's local voxel 0 (upper_global_first: of upper's).
int fvb_spatial_run::link_up(fvb_spatial_run &upper, int global_first, int upper_global_first)
{
    std::vector<int32_t> nn((size_t)V * 6);
    FVB_HIP_CHECK(hipMemcpyAsync(nn.data(), d_nn.p, sizeof(int32_t) * nn.size(), hipMemcpyDeviceToHost, stream));
    FVB_HIP_CHECK(hipStreamSynchronize(stream));
    std::vector<int32_t> up_pos((size_t)sa.n_pos, -1);
    for (int v = owned_begin; v < owned_end; v++)
        for (int a = 0; a < 6; a++)
        {
            const int u = nn[(size_t)v * 6 + a];
            if (u < owned_end)
                continue; // (none, or not a ghost above)
            const long long in_upper = (long long)global_first + u - upper_global_first;
            if (in_upper < upper.owned_begin || in_upper >= upper.owned_end)
                return api_fail(-49, "slab decomposition: a ghost voxel is not owned by the slab above");
            up_pos[(size_t)h_pos_of[(size_t)v]] = upper.h_pos_of[(size_t)in_upper];
        }
    FVB_HIP_CHECK(d_up_pos.alloc(sizeof(int32_t) * up_pos.size(), stream));
    FVB_HIP_CHECK(hipMemcpyAsync(d_up_pos.p, up_pos.data(), sizeof(int32_t) * up_pos.size(), hipMemcpyHostToDevice, stream));
    sa.sw_up_pos = (const int32_t *)d_up_pos.p;
    sa.sw_gran_up = upper.sa.sw_gran;
    sa.up_n_pos = upper.sa.n_pos;
    FVB_HIP_CHECK(hipMemcpyAsync(d_sa.p, &sa, sizeof(SpatialArgs), hipMemcpyHostToDevice, stream));
    FVB_HIP_CHECK(hipStreamSynchronize(stream)); // (up_pos is a local)
    return 0;
}

int fvb_spatial_run::sweep_fast(int it)
{
    int rc = fast_prep(it);
    if (rc == 0)
        rc = fast_sweep();
    return rc ? rc : fast_noise(it);
}

int fvb_spatial_run::fast_failed(bool &failed)
{
    failed = false;
    if (!fast)
        return 0;
    int32_t flag = 0;
    FVB_HIP_CHECK(hipMemcpyAsync(&flag, sa.sw_flags, sizeof(flag), hipMemcpyDeviceToHost, stream));
    FVB_HIP_CHECK(hipStreamSynchronize(stream));
    failed = flag != 0;
    return 0;
}

int fvb_spatial_run::copy_means(int v_begin, int v_count, double *host_means, int32_t *host_status, bool to_device)
{
    if (v_begin < 0 || v_count < 0 || v_begin + v_count > V)
        return api_fail(-46, "voxel range outside the local voxel list");
    if (v_count == 0)
        return 0;
    // rows 0..P-1 of the state image are the posterior means (SpLayout::M)
    double *dev = (double *)d_state.p + v_begin;
    const size_t width = sizeof(double) * (size_t)v_count;
    if (host_means)
    {
        if (to_device)
            FVB_HIP_CHECK(copy_rows(dev, sizeof(double) * (size_t)V, host_means, width, width, P, hipMemcpyDefault, stream));
        else
            FVB_HIP_CHECK(copy_rows(host_means, width, dev, sizeof(double) * (size_t)V, width, P, hipMemcpyDefault, stream));
    }
    if (host_status)
    {
        int32_t *ds = (int32_t *)d_status.p + v_begin;
        if (to_device)
            FVB_HIP_CHECK(hipMemcpyAsync(ds, host_status, sizeof(int32_t) * (size_t)v_count, hipMemcpyDefault, stream));
        else
            FVB_HIP_CHECK(hipMemcpyAsync(host_status, ds, sizeof(int32_t) * (size_t)v_count, hipMemcpyDefault, stream));
    }
    FVB_HIP_CHECK(hipStreamSynchronize(stream));
    return 0;
}

int fvb_spatial_run::finish()
{
    sa.it = cfg.max_iterations;
    hipLaunchKernelGGL(k.pack, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, stream, sa);
    FVB_HIP_CHECK(hipGetLastError());
    FVB_HIP_CHECK(hipStreamSynchronize(stream)); // the work buffers are freed with the object
    return 0;
}

namespace
{
// A model that is evaluated on the host (FVB_MODEL_HOSTJAC) under spatial VB: the two places of the loop that
// run the model - the set-up re-centre and the re-centre that ends every iteration's second sweep
// (inference_vb.cc:235,695) - become a call of the caller's linearisation callback for the voxels still
// taking part, about the means the first sweep left, and an upload of g and J; the kernels read them through
// HostLinModel. Two device buffers [V][T (P + 1)]: the second sweep needs the linearisation about the OLD
// centre for k = y - g + J (centre - mean) next to the new one.
struct HostLin
{
    fvb_linearise_fn linearise = nullptr;
    void *user = nullptr;
    const double *init_means = nullptr; // host, [V][P]: the centres of the set-up re-centre
    size_t V = 0, T = 0;
    int P = 0;
    DevMem buf[2];
    int cur = 0; // buf[cur] belongs to the moments in the state
    std::vector<double> lin, means_rows, means;
    std::vector<int32_t> status, ids;
    size_t stride() const
    {
        return T * (size_t)(P + 1);
    }
    int open(const fvb_config *cfg, hipStream_t stream)
    {
        V = (size_t)cfg->n_voxels;
        T = (size_t)cfg->n_times;
        P = cfg->n_params;
        const double bytes = (double)V * stride() * sizeof(double);
        if (bytes > 48e9)
            return api_fail(-55, "host-evaluated model under spatial VB: two linearisation buffers of " + std::to_string((long long)(bytes / 1e9))
                + " GB each do not fit the budget (48 GB each)");
        if (getenv("FVB_SPATIAL_VERBOSE") || bytes > 4e9)
            fprintf(stderr, "[fvb spatial] host-evaluated model: the linearisations of the whole volume are resident twice on the device "
                            "and once on the host, %.2f GB each\n", bytes / 1e9);
        for (int i = 0; i < 2; i++)
            FVB_HIP_CHECK(buf[i].alloc(sizeof(double) * V * stride(), stream));
        lin.resize(V * stride());
        return 0;
    }
    // g and J of the voxels with status 0 about means [V][P] (voxel-major) into buf[which]
    int relinearise(const double *centres, const int32_t *voxel_status, int which, hipStream_t stream)
    {
        ids.clear();
        for (size_t v = 0; v < V; v++)
            if (!voxel_status || voxel_status[v] == 0)
                ids.push_back((int32_t)v);
        if (ids.empty())
            return 0;
        const bool all = ids.size() == V;
        const double *active = centres;
        if (!all)
        {
            means.resize(ids.size() * (size_t)P);
            for (size_t a = 0; a < ids.size(); a++)
                for (int i = 0; i < P; i++)
                    means[a * P + i] = centres[(size_t)ids[a] * P + i];
            active = means.data();
        }
        const int cb = linearise(user, (int32_t)ids.size(), ids.data(), active, lin.data());
        if (cb != 0)
            return api_fail(-54, "the model's linearisation callback failed (code " + std::to_string(cb) + ")");
        if (!all) // spread the active voxels' blocks out to their own places (back to front: in place)
            for (size_t a = ids.size(); a-- > 0;)
                if ((size_t)ids[a] != a)
                    memmove(lin.data() + (size_t)ids[a] * stride(), lin.data() + a * stride(), sizeof(double) * stride());
        FVB_HIP_CHECK(hipMemcpyAsync(buf[which].p, lin.data(), sizeof(double) * V * stride(), hipMemcpyHostToDevice, stream));
        FVB_HIP_CHECK(hipStreamSynchronize(stream));
        return 0;
    }
};

int run_spatial(const fvb_config *cfg, const fvb_spatial *sp, const void *d_data, const fvb_outputs *d_out,
    hipStream_t stream, void (*progress_cb)(int, int), bool allow_fast = true, HostLin *hl = nullptr)
{
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    const auto t_start = now();
    fvb_spatial_run run;
    run.allow_fast = allow_fast && !hl; // (a host model's means must be complete before the second sweep starts)
    int rc;
    if (hl)
    {
        if ((rc = hl->open(cfg, stream)) != 0 || (rc = hl->relinearise(hl->init_means, nullptr, 0, stream)) != 0)
            return rc;
        hl->cur = 0;
        run.lin_cur = run.lin_next = (const double *)hl->buf[0].p;
    }
    rc = run.open(cfg, sp, d_data, d_out, stream);
    if (rc)
        return rc;
    const auto t_open = now();
    for (int it = 0; it < cfg->max_iterations; it++)
    {
        if (progress_cb)
            progress_cb(it, cfg->max_iterations); // inference_vb.cc:610
        if (run.has_spatial && (it > 0 || sp->update_first_iter))
        {
            if ((rc = run.ak_sums(nullptr)) != 0 || (rc = run.set_ak_sums(nullptr)) != 0)
                return rc;
        }
        if (hl)
        {
            // first sweep; the model about the new means (host); second sweep
            if ((rc = run.sweep_levels(it, LLONG_MIN, LLONG_MAX)) != 0)
                return rc;
            const size_t V = hl->V;
            const int P = hl->P;
            hl->means_rows.resize(V * (size_t)P);
            hl->status.resize(V);
            if ((rc = run.copy_means(0, (int)V, hl->means_rows.data(), hl->status.data(), false)) != 0)
                return rc;
            std::vector<double> centres(V * (size_t)P); // [V][P]
            for (int i = 0; i < P; i++)
                for (size_t v = 0; v < V; v++)
                    centres[v * P + i] = hl->means_rows[(size_t)i * V + v];
            const int spare = 1 - hl->cur;
            if ((rc = hl->relinearise(centres.data(), hl->status.data(), spare, stream)) != 0)
                return rc;
            run.sa.lin_cur = (const double *)hl->buf[hl->cur].p;
            run.sa.lin_next = (const double *)hl->buf[spare].p;
            if ((rc = run.sweep_noise(it)) != 0)
                return rc;
            hl->cur = spare;
            continue;
        }
        if ((rc = (run.fast ? run.sweep_fast(it) : run.sweep(it))) != 0)
            return rc;
    }
    bool failed = false;
    if ((rc = run.fast_failed(failed)) != 0)
        return rc;
    if (failed)
    {
        // a voxel failed DURING a first sweep (or the sweep's barrier gave up): the split sweep does not
        // reproduce what that does to the voxels after it. Nothing has been written to the outputs that the
        // repeat does not overwrite: do the run again with the per-level launches.
        if (run.env.timing || run.env.verbose)
            fprintf(stderr, "[fvb spatial] split first sweep abandoned, repeating the run with per-level launches\n");
        return run_spatial(cfg, sp, d_data, d_out, stream, nullptr, false);
    }
    const auto t_enq = now();
    if ((rc = run.finish()) != 0)
        return rc;
    if (run.env.timing)
        fprintf(stderr, "[fvb spatial] V=%d levels/runs=%zu: geometry %.1f ms (neighbours %.1f), alloc+upload+setup %.1f ms, enqueue %.1f ms, drain %.1f ms\n",
            run.V, run.slab_form ? run.level_begin_counts.size() : run.level_begin.size() - 1, run.t_geometry_ms, run.t_neighbours_ms, ms(t_start, t_open) - run.t_geometry_ms, ms(t_open, t_enq),
            ms(t_enq, now()));
    return 0;
}
} // namespace

extern "C" {

int32_t fabber_vb_register_device_spatial_model(const fvb_device_spatial_model *model)
{
    return DeviceRegistry<fvb_device_spatial_model>::instance().add(model);
}

int32_t fabber_vb_unregister_device_spatial_model(const char *name, int32_t n_params)
{
    return DeviceRegistry<fvb_device_spatial_model>::instance().remove(name, n_params);
}

int32_t fabber_vb_device_spatial_model_count(void)
{
    return DeviceRegistry<fvb_device_spatial_model>::instance().count();
}

const char *fabber_vb_device_spatial_model_name(int32_t i)
{
    return DeviceRegistry<fvb_device_spatial_model>::instance().name(i);
}

int32_t fabber_vb_device_spatial_model_params(int32_t i)
{
    return DeviceRegistry<fvb_device_spatial_model>::instance().params(i, 0);
}

int32_t fabber_vb_register_device_spatial_noise_model(const fvb_device_spatial_noise_model *model)
{
    return DeviceRegistry<fvb_device_spatial_noise_model>::instance().add(model);
}

int32_t fabber_vb_unregister_device_spatial_noise_model(const char *name, int32_t n_params)
{
    return DeviceRegistry<fvb_device_spatial_noise_model>::instance().remove(name, n_params);
}

int32_t fabber_vb_device_spatial_noise_model_count(void)
{
    return DeviceRegistry<fvb_device_spatial_noise_model>::instance().count();
}

const char *fabber_vb_device_spatial_noise_model_name(int32_t i)
{
    return DeviceRegistry<fvb_device_spatial_noise_model>::instance().name(i);
}

int32_t fabber_vb_device_spatial_noise_model_params(int32_t i)
{
    return DeviceRegistry<fvb_device_spatial_noise_model>::instance().params(i, 0);
}

int32_t fabber_vb_find_device_spatial_noise_model(const char *name, int32_t n_params, fvb_device_spatial_noise_model *entry)
{
    return (name && entry && DeviceRegistry<fvb_device_spatial_noise_model>::instance().find(name, n_params, entry)) ? 1 : 0;
}

int32_t fabber_vb_register_device_spatial_wave_model(const fvb_device_spatial_wave_model *model)
{
    return DeviceRegistry<fvb_device_spatial_wave_model>::instance().add(model);
}

int32_t fabber_vb_unregister_device_spatial_wave_model(const char *name)
{
    return DeviceRegistry<fvb_device_spatial_wave_model>::instance().remove(name, 0);
}

int32_t fabber_vb_device_spatial_wave_model_count(void)
{
    return DeviceRegistry<fvb_device_spatial_wave_model>::instance().count();
}

const char *fabber_vb_device_spatial_wave_model_name(int32_t i)
{
    return DeviceRegistry<fvb_device_spatial_wave_model>::instance().name(i);
}

int32_t fabber_vb_find_device_spatial_wave_model(const char *name, fvb_device_spatial_wave_model *entry)
{
    return (name && entry && DeviceRegistry<fvb_device_spatial_wave_model>::instance().find(name, 0, entry)) ? 1 : 0;
}

int32_t fabber_vb_register_device_spatial_wave_ar_model(const fvb_device_spatial_wave_ar_model *model)
{
    return DeviceRegistry<fvb_device_spatial_wave_ar_model>::instance().add(model);
}

int32_t fabber_vb_unregister_device_spatial_wave_ar_model(const char *name)
{
    return DeviceRegistry<fvb_device_spatial_wave_ar_model>::instance().remove(name, 0);
}

int32_t fabber_vb_device_spatial_wave_ar_model_count(void)
{
    return DeviceRegistry<fvb_device_spatial_wave_ar_model>::instance().count();
}

const char *fabber_vb_device_spatial_wave_ar_model_name(int32_t i)
{
    return DeviceRegistry<fvb_device_spatial_wave_ar_model>::instance().name(i);
}

int32_t fabber_vb_find_device_spatial_wave_ar_model(const char *name, fvb_device_spatial_wave_ar_model *entry)
{
    return (name && entry && DeviceRegistry<fvb_device_spatial_wave_ar_model>::instance().find(name, 0, entry)) ? 1 : 0;
}

int32_t fabber_vb_register_device_spatial_wave_noise_model(const fvb_device_spatial_wave_noise_model *model)
{
    return DeviceRegistry<fvb_device_spatial_wave_noise_model>::instance().add(model);
}

int32_t fabber_vb_unregister_device_spatial_wave_noise_model(const char *name)
{
    return DeviceRegistry<fvb_device_spatial_wave_noise_model>::instance().remove(name, 0);
}

int32_t fabber_vb_device_spatial_wave_noise_model_count(void)
{
    return DeviceRegistry<fvb_device_spatial_wave_noise_model>::instance().count();
}

const char *fabber_vb_device_spatial_wave_noise_model_name(int32_t i)
{
    return DeviceRegistry<fvb_device_spatial_wave_noise_model>::instance().name(i);
}

int32_t fabber_vb_find_device_spatial_wave_noise_model(const char *name, fvb_device_spatial_wave_noise_model *entry)
{
    return (name && entry && DeviceRegistry<fvb_device_spatial_wave_noise_model>::instance().find(name, 0, entry)) ? 1 : 0;
}

// (the selection function of the run: "" where open() would answer -40 or -44)
const char *fabber_vb_spatial_kernel_name(const fvb_config *cfg)
{
    if (!cfg || cfg->abi_version != FVB_ABI_VERSION || cfg->n_params <= 0)
        return "";
    const SpatialRoute route = spatial_kernels_for(cfg);
    if (!route.found())
        return "";
    g_spatial_kernel_name = route.name;
    return g_spatial_kernel_name.c_str();
}

// the argument checks of the device entry points
static int32_t spatial_check_args(const fvb_config *cfg, const fvb_spatial *sp, const fvb_outputs *out)
{
    int rc = api_validate(cfg, true);
    if (rc)
        return rc;
    if (!sp || !sp->coords)
        return api_fail(-42, "spatial description / coordinates missing");
    if (sp->spatial_dims < 0 || sp->spatial_dims > 3)
        return api_fail(-43, "spatial-dims must be 0, 1, 2 or 3");
    if (spatial_noise_kind(cfg) < 0)
        return api_fail(-44, spatial_noise_refusal);
    if (!out || !out->mvn)
        return api_fail(-20, "outputs.mvn is required");
    return 0;
}

static int32_t run_spatial_checked(const fvb_config *cfg, const fvb_spatial *sp, const void *data, const fvb_outputs *out, void *stream,
    void (*progress_cb)(int, int), HostLin *hl)
{
    int rc = spatial_check_args(cfg, sp, out);
    if (rc)
        return rc;
    if (cfg->n_voxels == 0)
        return 0;
    if (!data)
        return api_fail(-21, "data is NULL");
    return run_spatial(cfg, sp, data, out, (hipStream_t)stream, progress_cb, true, hl);
}

int32_t fabber_vb_run_spatial_device(const fvb_config *cfg, const fvb_spatial *sp, const void *data,
    const fvb_outputs *out, void *stream, void (*progress_cb)(int, int))
{
    if (cfg && cfg->model == FVB_MODEL_HOSTJAC)
        return api_fail(-56, "a model evaluated on the host runs spatial VB through fabber_vb_run_spatial_hostmodel_host");
    return run_spatial_checked(cfg, sp, data, out, stream, progress_cb, nullptr);
}

int32_t fabber_vb_spatial_open(const fvb_config *cfg, const fvb_spatial *sp, const void *data, const fvb_outputs *out,
    void *stream, fvb_spatial_run **run)
{
    if (!run)
        return api_fail(-47, "run handle pointer is NULL");
    *run = nullptr;
    int rc = spatial_check_args(cfg, sp, out);
    if (rc)
        return rc;
    if (cfg->n_voxels == 0 || !data)
        return api_fail(-21, "no voxels / data is NULL");
    fvb_spatial_run *r = new fvb_spatial_run();
    rc = r->open(cfg, sp, data, out, (hipStream_t)stream);
    if (rc)
    {
        delete r;
        return rc;
    }
    *run = r;
    return 0;
}

int32_t fabber_vb_spatial_ak_sums(fvb_spatial_run *run, double *sums)
{
    return run ? run->ak_sums(sums) : api_fail(-47, "run handle is NULL");
}

int32_t fabber_vb_spatial_ak_segment_sums(fvb_spatial_run *run, double *partials, int32_t *n_segments)
{
    if (!run || !n_segments)
        return api_fail(-47, "run handle is NULL");
    *n_segments = run->n_segments;
    return partials ? run->ak_segment_sums(partials) : 0;
}

int32_t fabber_vb_spatial_set_ak_sums(fvb_spatial_run *run, const double *sums)
{
    return run ? run->set_ak_sums(sums) : api_fail(-47, "run handle is NULL");
}

int32_t fabber_vb_spatial_sweep(fvb_spatial_run *run, int32_t iteration)
{
    return run ? run->sweep(iteration) : api_fail(-47, "run handle is NULL");
}

int32_t fabber_vb_spatial_sweep_levels(fvb_spatial_run *run, int32_t iteration, int64_t level_lo, int64_t level_hi)
{
    return run ? run->sweep_levels(iteration, level_lo, level_hi) : api_fail(-47, "run handle is NULL");
}

int32_t fabber_vb_spatial_sweep_noise(fvb_spatial_run *run, int32_t iteration)
{
    return run ? run->sweep_noise(iteration) : api_fail(-47, "run handle is NULL");
}

int32_t fabber_vb_spatial_level_weights(fvb_spatial_run *run, int32_t weights[3])
{
    if (!run || !weights)
        return api_fail(-47, "run handle is NULL");
    for (int i = 0; i < 3; i++)
        weights[i] = run->level_w[i];
    return 0;
}

int32_t fabber_vb_spatial_fprior(fvb_spatial_run *run, double *value, int32_t set)
{
    if (!run || !value)
        return api_fail(-47, "run handle is NULL");
    hipError_t e = set ? hipMemcpyAsync(run->d_fprior.p, value, sizeof(double), hipMemcpyDefault, run->stream)
                       : hipMemcpyAsync(value, run->d_fprior.p, sizeof(double), hipMemcpyDefault, run->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(run->stream);
    return e == hipSuccess ? 0 : api_fail(-100 - (int)e, hipGetErrorString(e));
}

int32_t fabber_vb_spatial_copy_means(fvb_spatial_run *run, int32_t v_begin, int32_t v_count, double *means, int32_t *status,
    int32_t to_device)
{
    return run ? run->copy_means(v_begin, v_count, means, status, to_device != 0) : api_fail(-47, "run handle is NULL");
}

int32_t fabber_vb_spatial_close(fvb_spatial_run *run)
{
    if (!run)
        return api_fail(-47, "run handle is NULL");
    const int rc = run->finish();
    delete run;
    return rc;
}

static int32_t run_spatial_host_impl(const fvb_config *cfg, const fvb_spatial *sp, const void *data, const fvb_outputs *out,
    int32_t device, void (*progress_cb)(int, int), HostLin *hl)
{
    int rc = api_validate(cfg, true);
    if (rc)
        return rc;
    if (!out || !out->mvn)
        return api_fail(-20, "outputs.mvn is required");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return api_fail(-30, "no HIP device available (the VB engine has no CPU fallback)");
    FVB_HIP_CHECK(hipSetDevice(device));
    const size_t V = (size_t)cfg->n_voxels;
    if (V == 0)
        return 0;
    // (before anything is uploaded: a caller that falls back to the host-evaluated route on -40 has not paid for the
    // series on the device twice)
    if (spatial_noise_kind(cfg) < 0)
        return api_fail(-44, spatial_noise_refusal);
    if (!spatial_kernels_for(cfg).found())
        return api_fail(-40, spatial_kernels_refusal(cfg));
    if (cfg->model == FVB_MODEL_PLUGIN && !cfg->init_mvn && !find_init_entry(cfg)) // (with an entry: fvb_spatial_run::open)
        return api_fail(-52, spatial_init_mvn_refusal);
    const int P = cfg->n_params;
    const int n = P + noise_outputs(cfg), rows = n * (n + 1) / 2 + n + 1;
    StagedProblem staged;
    if ((rc = staged.stage_in(cfg, data, out, (size_t)rows, 0, V, nullptr, from_pool(), STAGE_SPATIAL)) != 0)
        return rc;
    if (staged.dout.free_energy) // NaN: a voxel that fails before any F is evaluated keeps it
        FVB_HIP_CHECK(hipMemset(staged.dout.free_energy, 0xff, sizeof(double) * V));
    fvb_spatial dsp = *sp;
    DevMem b_locked;
    if (sp->locked_centres)
    {
        if ((rc = upload_array(b_locked, sp->locked_centres, sizeof(double) * P * V, nullptr)) != 0)
            return rc;
        dsp.locked_centres = (const double *)b_locked.p;
    }
    rc = run_spatial_checked(&staged.d, &dsp, staged.b_data.p, &staged.dout, nullptr, progress_cb, hl);
    if (rc)
        return rc;
    FVB_HIP_CHECK(hipDeviceSynchronize());
    return staged.stage_out(out, nullptr);
}

int32_t fabber_vb_run_spatial_host(const fvb_config *cfg, const fvb_spatial *sp, const void *data,
    const fvb_outputs *out, int32_t device, void (*progress_cb)(int, int))
{
    if (cfg && cfg->model == FVB_MODEL_HOSTJAC)
        return api_fail(-56, "a model evaluated on the host runs spatial VB through fabber_vb_run_spatial_hostmodel_host");
    return run_spatial_host_impl(cfg, sp, data, out, device, progress_cb, nullptr);
}

int32_t fabber_vb_run_spatial_hostmodel_host(const fvb_config *cfg, const fvb_spatial *sp, const void *data, const fvb_outputs *out,
    int32_t device, fvb_linearise_fn linearise, void *user, void (*progress_cb)(int, int))
{
    if (!cfg || cfg->model != FVB_MODEL_HOSTJAC)
        return api_fail(-56, "fabber_vb_run_spatial_hostmodel_host is for cfg->model = FVB_MODEL_HOSTJAC");
    if (!linearise)
        return api_fail(-50, "linearisation callback is NULL");
    if (!cfg->init_mvn)
        return api_fail(-52, "host-evaluated models need the initial posterior as init_mvn (the model's InitVoxelPosterior runs on the host)");
    if (sp && sp->locked_centres)
        return api_fail(-57, "locked linearisation centres are not available for host-evaluated models under spatial VB");
    // the centres of the set-up re-centre: the means of the initial posterior, voxel-major
    const size_t V = (size_t)cfg->n_voxels;
    const int P = cfg->n_params, n = P + noise_outputs(cfg), nCov = n * (n + 1) / 2;
    std::vector<double> init_means(V * (size_t)P);
    for (size_t v = 0; v < V; v++)
        for (int i = 0; i < P; i++)
            init_means[v * P + i] = cfg->init_mvn[(size_t)(nCov + i) * V + v];
    HostLin hl;
    hl.linearise = linearise;
    hl.user = user;
    hl.init_means = init_means.data();
    return run_spatial_host_impl(cfg, sp, data, out, device, progress_cb, &hl);
}

} // extern "C"

// Host-only helper (no GPU needed): the first-neighbour table the spatial driver builds,
// [n_voxels][6], 0-based ids, -1 = none. For the unit tests of the neighbour construction.
extern "C" int32_t fabber_vb_neighbours(const int32_t *coords, int32_t n_voxels, int32_t spatial_dims, int32_t *nn_out)
{
    std::vector<int32_t> nn;
    std::string err = plan::build_neighbours(coords, n_voxels, spatial_dims, nn);
    if (!err.empty())
        return fvb::api_fail(-41, err);
    std::copy(nn.begin(), nn.end(), nn_out);
    return 0;
}
