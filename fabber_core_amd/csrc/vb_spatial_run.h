/*
 * vb_spatial_run.h - one spatial VB run on one device (fvb_spatial_run, defined in vb_spatial_api.hip) as the driver
 * of a run on several devices sees it (vb_spatial_multi.hip), the environment switches of the spatial host layer and
 * the few helpers the two sources share. Host code only: no kernel includes this file.
 */
#pragma once

#include "vb_spatial_noise.h"
#include "vb_host_stage.h"
#include "vb_spatial_plan.h"

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

namespace fvb
{
static_assert(plan::NP_BELOW == FVB_NP_BELOW && plan::NP_ABOVE == FVB_NP_ABOVE, "ghost markers of the planner and the kernels");

// The environment switches of the spatial host layer, read at the top of every open / execute call:
// tests change them between runs.
struct SpatialEnv
{
    bool host_geometry = false, per_level = false, host_numbering = false, prep_linear = false;
    bool timing = false, verbose = false, multi_serial = false, multi_pipeline = false;
    plan::Forced host_threads, slab_dz, slab_width, chunk_levels;
    static SpatialEnv read()
    {
        auto flag = [](const char *name) { return getenv(name) != nullptr; };
        auto forced = [](const char *name) {
            plan::Forced f;
            if (const char *v = getenv(name))
            {
                f.set = true;
                f.value = atoi(v);
            }
            return f;
        };
        SpatialEnv e;
        e.host_geometry = flag("FVB_SPATIAL_HOST_GEOMETRY");
        e.per_level = flag("FVB_SPATIAL_PER_LEVEL");
        e.host_numbering = flag("FVB_SPATIAL_HOST_NUMBERING");
        e.prep_linear = flag("FVB_SPATIAL_PREP_LINEAR");
        e.timing = flag("FVB_SPATIAL_TIMING");
        e.verbose = flag("FVB_SPATIAL_VERBOSE");
        e.multi_serial = flag("FVB_SPATIAL_MULTI_SERIAL");
        e.multi_pipeline = flag("FVB_SPATIAL_MULTI_PIPELINE");
        e.host_threads = forced("FVB_SPATIAL_HOST_THREADS");
        e.slab_dz = forced("FVB_SPATIAL_SLAB_DZ");
        e.slab_width = forced("FVB_SPATIAL_SLAB_WIDTH");
        e.chunk_levels = forced("FVB_SPATIAL_CHUNK_LEVELS");
        return e;
    }
};

// the map from box offsets to voxels the neighbour table's kernels leave (the prep kernel's tiles read it)
struct DenseMap
{
    DevMem map; // [span] voxel at box offset base + i, -1 = none
    long long base = 0, span = 0;
    int xsize = 0, ysize = 0;
};

// vb_spatial_api.hip
// Which statistics a configuration's state image carries (vb_spatial_noise.h), or -1: no spatial kernels for it
int spatial_noise_kind(const fvb_config *cfg);
extern const char *const spatial_noise_refusal;
} // namespace fvb

// One spatial VB run on one device: geometry, work buffers and the per-iteration steps. A single
// process drives it from run_spatial(); with several slabs the caller interleaves the steps
// with its collectives (all-reduce of the a_K sums, halo exchange of the boundary planes).
struct fvb_spatial_run
{
    fvb_config cfg;
    fvb_spatial sp;
    fvb::SpatialEnv env;
    fvb::SpatialKernels k;
    // a body of a model library (FVB_MODEL_PLUGIN): the launcher of its spatial entry. The three kernels of the family
    // that evaluate the model - set-up and the second sweep in its two forms - are the library's then and k's slots for
    // them are NULL; everything else in k is the engine's own for the parameter count
    fvb_device_spatial_launch_fn library = nullptr;
    // ... or, under a noise pattern or AR(1) noise, of its entry for these policies, which is told the noise kind
    fvb_device_spatial_noise_launch_fn library_noise = nullptr;
    int library_kind = 0;
    fvb::SpatialArgs sa;
    hipStream_t stream = nullptr;
    int V = 0, P = 0, owned_begin = 0, owned_end = 0;
    bool has_spatial = false;
    size_t noise_lds = 0; // dynamic LDS of the set-up and second-sweep kernels (noise-pattern: the class of every timepoint)
    std::vector<int32_t> level_begin;
    std::vector<long long> level_value; // the level (weighted co-ordinate sum) of each entry of level_begin
    int level_w[3] = { 1, 1, 1 };
    fvb::DevMem d_state, d_nn, d_nn_dir, d_order, d_aK, d_partials, d_fprior, d_status, d_sa, d_sums, d_seg_start;
    // the initial posterior of a library body that came without init_mvn, written by the library's initial-posterior
    // kernel (include/fabber_device_init_model.h); cfg.init_mvn points here then
    fvb::DevMem d_init_mvn;
    int n_segments = 0;
    double t_geometry_ms = 0, t_neighbours_ms = 0;
    // the split first sweep (vb_spatial.h): whole-volume runs, or one of several slabs that sweep together
    bool allow_fast = false, fast = false;
    bool multi_fast = false; // one of several slabs on several devices that sweep together (fabber_vb_run_spatial_host_multi)
    int device_share = 1;    // how many such slabs run on THIS device at once (a device listed several times)
    bool gran_fine = false;  // multi_fast: the inboxes are fine-grained memory (another DEVICE may write them)
    fvb::DevMem d_up_pos;
    fvb::DenseMap dense; // (kept from the neighbour table's kernels)
    std::vector<int32_t> h_pos_of; // (multi_fast: the numbering, for the slab below to address this slab's inboxes)
    int fast_prep(int it);
    int fast_sweep();
    int fast_noise(int it);
    int link_up(fvb_spatial_run &upper, int global_first, int upper_global_first);
    std::vector<int32_t> level_begin_counts; // voxels per level
    fvb::DevMem d_pos_of, d_level_pos, d_level_count, d_sw_f64, d_sw_i32, d_sw_sync, d_sw_gran, d_slab_first;
    int max_runs_per_slab = 0;
    bool slab_form = false; // (= fast) the voxels are numbered slab-major for vb_spatial_slab_sweep_kernel
    int sweep_fast(int it);
    int fast_failed(bool &failed);
    // the second-sweep kernel of iteration `it`: the instance with the half-ulp exp where the iteration ends in one
    // of the run's pointwise linearisations (vb_spatial.h: sp_precise) and such an instance was built
    fvb::SpatialKernelFn second_sweep(bool fast_form, int it) const
    {
        const bool pointwise = it + 1 < sa.ka.precise_passes && !sa.locked_linear;
        fvb::SpatialKernelFn acc = fast_form ? k.noise_fast_acc : k.noise_acc;
        return (pointwise && acc) ? acc : (fast_form ? k.noise_fast : k.noise);
    }
    // host-evaluated models: the linearisations the set-up re-centre reads (see HostLin in vb_spatial_api.hip)
    const double *lin_cur = nullptr, *lin_next = nullptr;
    hipStream_t setup_stream = nullptr;
    int setup_device = 0;
    hipEvent_t setup_done = nullptr;
    ~fvb_spatial_run()
    {
        if (setup_stream)
        {
            (void)hipStreamSynchronize(setup_stream); // (before the buffers its kernel writes are given back)
            fvb::api_return_side_stream(setup_stream, setup_device); // (kept for the next run on this device)
        }
        if (setup_done)
            (void)hipEventDestroy(setup_done);
    }

    int open(const fvb_config *cfg_, const fvb_spatial *sp_, const void *d_data, const fvb_outputs *d_out, hipStream_t stream_);
    // the steps of open(), in order; Geometry is what they hand on (vb_spatial_api.hip)
    struct Geometry;
    int start_setup(const void *d_data, const fvb_outputs *d_out);
    int neighbour_table(Geometry &g);
    int plan_sweeps(Geometry &g);
    int number_slabs_device(Geometry &g, const fvb::plan::Levels &lv, long long slab_cap);
    int upload_plan(Geometry &g);
    int upload_slab_form(const Geometry &g);
    int publish_args();

    int ak_sums(double *host_sums);
    int ak_segment_sums(double *host_partials);
    int set_ak_sums(const double *host_sums);
    int sweep(int it);
    int sweep_levels(int it, long long lo, long long hi);
    int sweep_noise(int it);
    // the one launch of a kernel that evaluates the model (which: FVB_SPATIAL_KERNEL_*; fn: the engine's own kernel for it)
    int launch_model_kernel(int which, fvb::SpatialKernelFn fn, unsigned grid, size_t lds, hipStream_t on);
    int copy_means(int v_begin, int v_count, double *host_means, int32_t *host_status, bool to_device);
    int finish();
};
