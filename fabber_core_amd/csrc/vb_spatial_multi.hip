/*
 * vb_spatial_multi.hip - spatial VB of one volume on several devices, driven by this one process.
 * The decomposition and the schedule of fabber_core_amd/spatial_mgpu.py (one process per GPU over
 * torch.distributed) inside the engine: z-slabs with ghost planes, the first sweep as a pipeline over chunks
 * of 16 global levels (slab r sweeps chunk c at tick c + r and hands its top planes to slab r + 1 after every
 * tick), the a_K sums added over the segments of the voxel list in voxel order, the prior term of the last
 * voxel from the last slab, the second sweep, the exchange of the boundary planes both ways. The result is the
 * single-device run bit for bit (tests/test_spatial_mgpu.py). Planes travel device to device
 * (hipMemcpyPeerAsync between staging buffers; a device listed twice is a copy on itself).
 */
#include "vb_spatial_run.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

using namespace fvb;

extern "C" const char *fabber_vb_last_error(void);
namespace
{
struct SlabRun
{
    int dev = 0, g0 = 0, b = 0, e = 0, g1 = 0; // local list = global voxels [g0, g1), owned [b, e)
    hipStream_t stream = nullptr;
    StagedProblem staged; // its part of the problem: the local list
    fvb_spatial sp;
    std::vector<int32_t> coords;
    DevMem stage_means, stage_status;
    fvb_spatial_run *run = nullptr;
    ~SlabRun()
    {
        (void)hipSetDevice(dev);
        delete run; // (its buffers go back to this device's pool in its stream's order)
        staged.release(); // ... and this slab's, before the stream they are ordered on goes
        stage_means.reset();
        stage_status.reset();
        if (stream)
        {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
    }
};

// means and status of n voxels: slab `from`, local index v_from -> slab `to`, local index v_to
int slab_transfer(SlabRun &from, int v_from, SlabRun &to, int v_to, int n, int P)
{
    if (n <= 0)
        return 0;
    FVB_HIP_CHECK(hipSetDevice(from.dev));
    int rc = from.run->copy_means(v_from, n, (double *)from.stage_means.p, (int32_t *)from.stage_status.p, false);
    if (rc)
        return rc;
    // (in the receiving slab's stream: ordered before the copy into its state, which ends with a wait for that
    // stream - so the sender's staging buffer is free again on return; the sender's copy above has completed)
    FVB_HIP_CHECK(hipSetDevice(to.dev));
    FVB_HIP_CHECK(hipMemcpyPeerAsync(to.stage_means.p, to.dev, from.stage_means.p, from.dev, sizeof(double) * (size_t)P * n, to.stream));
    FVB_HIP_CHECK(hipMemcpyPeerAsync(to.stage_status.p, to.dev, from.stage_status.p, from.dev, sizeof(int32_t) * (size_t)n, to.stream));
    return to.run->copy_means(v_to, n, (double *)to.stage_means.p, (int32_t *)to.stage_status.p, true);
}

double ms_since(std::chrono::steady_clock::time_point a)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
}
} // namespace

static thread_local int s_unlink_pair = -1;
extern "C" void fabber_vb_test_unlink_slab_pair(int32_t pair)
{
    s_unlink_pair = pair;
}

// One volume on several devices, in three steps a caller can time apart: the slabs and their part of the problem on
// their devices (open), a complete run on the resident data - geometry, set-up, every iteration, result images packed
// on the devices - as often as asked (run), the owned voxels' results into the caller's images (results).
struct fvb_spatial_multi
{
    fvb_config cfg;
    fvb_spatial sp;
    SpatialEnv env;
    std::vector<int32_t> coords; // (a copy: sp.coords points here)
    std::vector<int> devs;
    int V = 0, T = 0, P = 0, world = 0, halo = 1, rows = 0, max_halo = 1;
    bool second = false, has_spatial = false, peers = true;
    std::vector<std::unique_ptr<SlabRun> > slabs;
    const char *route = "";
    double ms_open = 0, ms_setup = 0, ms_loop = 0;

    // body(r) for every slab, each on a host thread of its own; the first failure (code and message) is the caller's
    int for_each_slab(const std::function<int(int)> &body)
    {
        std::vector<int> rcs(slabs.size(), 0);
        std::vector<std::string> errs(slabs.size());
        auto work = [&](int r) {
            rcs[(size_t)r] = body(r);
            if (rcs[(size_t)r] != 0)
                errs[(size_t)r] = fabber_vb_last_error(); // (thread-local: carried to the caller's thread)
        };
        std::vector<std::thread> pool;
        const bool threads = !env.multi_serial;
        for (int r = 1; r < (int)slabs.size() && threads; r++)
            pool.emplace_back(work, r);
        work(0);
        for (int r = 1; r < (int)slabs.size() && !threads; r++)
            work(r);
        for (auto &th : pool)
            th.join();
        for (size_t r = 0; r < slabs.size(); r++)
            if (rcs[r] != 0)
                return api_fail(rcs[r], errs[r]);
        return 0;
    }
    int plan(const fvb_config *cfg_, const fvb_spatial *sp_, const int32_t *devices, int32_t n_devices);
    int upload(const void *data, const fvb_outputs *out);
    int execute(void (*progress_cb)(int, int), bool no_fast);
    int open_slabs(bool try_fast);
    int link_slabs();
    int sweep_together(void (*progress_cb)(int, int));
    int sweep_pipeline(void (*progress_cb)(int, int));
    int reduce_ak();
    int hand_down_fprior();
    int exchange_boundaries();
    int run(void (*progress_cb)(int, int));
    int download(const fvb_outputs *out);
    void release();
    ~fvb_spatial_multi()
    {
        release();
    }
};

void fvb_spatial_multi::release()
{
    // (giving a slab's memory back unmaps it: a thread per slab)
    std::vector<std::thread> pool;
    for (size_t r = 1; r < slabs.size(); r++)
        pool.emplace_back([this, r]() { slabs[r].reset(); });
    if (!slabs.empty())
        slabs[0].reset();
    for (auto &th : pool)
        th.join();
    slabs.clear();
}

// ---- the slabs: the devices, and plan::slab_cuts of the z-planes ----
int fvb_spatial_multi::plan(const fvb_config *cfg_, const fvb_spatial *sp_, const int32_t *devices, int32_t n_devices)
{
    cfg = *cfg_;
    sp = *sp_;
    V = cfg.n_voxels;
    T = cfg.n_times;
    P = cfg.n_params;
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0)
        return api_fail(-30, "no HIP device available (the VB engine has no CPU fallback)");
    if (devices)
    {
        if (n_devices <= 0)
            return api_fail(-31, "empty device list");
        for (int i = 0; i < n_devices; i++)
        {
            if (devices[i] < 0 || devices[i] >= visible)
                return api_fail(-31, "device index " + std::to_string(devices[i]) + " out of range (" + std::to_string(visible) + " visible)");
            devs.push_back(devices[i]);
        }
    }
    else
        for (int i = 0; i < visible; i++)
            devs.push_back(i);
    coords.assign(sp_->coords, sp_->coords + 3 * (size_t)V);
    sp.coords = coords.data();
    const plan::PriorScan priors = plan::scan_priors(P, cfg.prior_type, cfg.prior_prec, cfg.prior_mean);
    second = priors.second_neighbours;
    has_spatial = priors.has_spatial;
    // the slabs of a run that sweep together write into each other's memory: every pair of neighbours must be peers
    for (size_t r = 0; r + 1 < devs.size() && peers; r++)
        if (devs[r] != devs[r + 1])
        {
            int can = 0;
            peers = hipDeviceCanAccessPeer(&can, devs[r], devs[r + 1]) == hipSuccess && can != 0;
            (void)hipGetLastError();
        }
    // ghost planes: the split form reads first neighbours only (types P, p are local there, and their a_K sums are
    // over first neighbours, priors.cc:280-301); the level-chunk pipeline's per-level kernel - what a run falls back
    // to - sums second neighbours too, so a problem with such priors keeps two planes either way
    halo = second ? 2 : 1;
    const int32_t *Z = coords.data() + 2 * (size_t)V;
    std::vector<int> plane_start;
    if (!plan::plane_starts(Z, V, plane_start))
        return api_fail(-41, "Coordinate matrix must be in correct order to use adjacency-based priors.");
    const std::vector<plan::SlabCut> cuts = plan::slab_cuts(Z, V, plane_start, (int)devs.size(), halo);
    world = (int)cuts.size();
    slabs.clear();
    for (int r = 0; r < world && world > 1; r++)
    {
        std::unique_ptr<SlabRun> sl(new SlabRun);
        sl->dev = devs[r];
        sl->g0 = cuts[r].g0;
        sl->b = cuts[r].b;
        sl->e = cuts[r].e;
        sl->g1 = cuts[r].g1;
        slabs.push_back(std::move(sl));
    }
    const int n = P + noise_outputs(&cfg);
    rows = n * (n + 1) / 2 + n + 1;
    max_halo = plan::max_halo(cuts);
    return 0;
}

// ---- per slab: its part of the problem on its device (a host thread per slab: the devices work side by side) ----
int fvb_spatial_multi::upload(const void *data, const fvb_outputs *out)
{
    env = SpatialEnv::read();
    auto upload_slab = [&](int r) -> int {
        SlabRun &sl = *slabs[r];
        FVB_HIP_CHECK(hipSetDevice(sl.dev));
        FVB_HIP_CHECK(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
        hipStream_t st = sl.stream;
        const size_t Vl = (size_t)(sl.g1 - sl.g0);
        const int rc = sl.staged.stage_in(&cfg, data, out, (size_t)rows, (size_t)sl.g0, (size_t)sl.g1, st, from_pool(), STAGE_SPATIAL);
        if (rc)
            return rc;
        FVB_HIP_CHECK(sl.stage_means.alloc(sizeof(double) * (size_t)P * max_halo, st));
        FVB_HIP_CHECK(sl.stage_status.alloc(sizeof(int32_t) * (size_t)max_halo, st));
        FVB_HIP_CHECK(hipStreamSynchronize(st)); // (the uploads read pageable host memory)
        sl.coords.resize(3 * Vl);
        for (int dim = 0; dim < 3; dim++)
            std::copy(coords.begin() + (size_t)dim * V + sl.g0, coords.begin() + (size_t)dim * V + sl.g1, sl.coords.begin() + (size_t)dim * Vl);
        sl.sp = sp;
        sl.sp.coords = sl.coords.data();
        sl.sp.owned_begin = sl.b - sl.g0;
        sl.sp.owned_end = sl.e - sl.g0;
        sl.sp.n_voxels_global = V;
        return 0;
    };
    return for_each_slab(upload_slab);
}

// ---- a complete run on the resident data: set-up, the iterations, the packed result images (on the devices) ----
int fvb_spatial_multi::run(void (*progress_cb)(int, int))
{
    int rc = execute(progress_cb, false);
    s_unlink_pair = -1; // (the test hook holds for one attempt)
    if (rc == 1) // the slabs could not sweep together (or gave that up): the level-chunk pipeline, the exact form
        rc = execute(progress_cb, true);
    return rc;
}

// Returns 1 where the run has to be repeated as the level-chunk pipeline.
int fvb_spatial_multi::execute(void (*progress_cb)(int, int), bool no_fast)
{
    int rc;
    env = SpatialEnv::read();
    const auto t_begin = std::chrono::steady_clock::now();
    // all slabs sweep together with the slab form of the split sweep (vb_spatial.h) unless that was tried and abandoned,
    // the devices cannot reach each other's memory, or FVB_SPATIAL_PER_LEVEL asks for the level-chunk pipeline
    const bool try_fast = has_spatial && peers && !no_fast && !env.per_level && !env.multi_pipeline;
    if ((rc = open_slabs(try_fast)) != 0)
        return rc;
    ms_setup = ms_since(t_begin);
    const auto t_loop = std::chrono::steady_clock::now();
    bool all_fast = try_fast;
    for (int r = 0; r < world; r++)
    {
        all_fast = all_fast && slabs[r]->run->slab_form;
        // (an inbox another DEVICE writes into must be fine-grained memory, or its stores may stay invisible to the polls)
        if (r > 0 && slabs[r]->dev != slabs[r - 1]->dev)
            all_fast = all_fast && slabs[r]->run->gran_fine;
    }
    if (try_fast && !all_fast) // (a slab the slab form does not take: the level-chunk pipeline for the whole run)
        return 1;
    if ((rc = all_fast ? sweep_together(progress_cb) : sweep_pipeline(progress_cb)) != 0)
        return rc;
    // ---- every slab packs its voxels' results (on its device) ----
    for (int r = 0; r < world; r++)
    {
        FVB_HIP_CHECK(hipSetDevice(slabs[r]->dev));
        if ((rc = slabs[r]->run->finish()) != 0) // (ends with a wait for the slab's stream)
            return rc;
    }
    ms_loop = ms_since(t_loop);
    route = all_fast ? "all slabs sweep together" : "level-chunk pipeline";
    if (env.timing)
        fprintf(stderr, "[fvb spatial] %d slabs (%s): geometry + set-up %.1f ms, %d iterations + result images %.1f ms\n", world, route, ms_setup,
            cfg.max_iterations, ms_loop);
    return 0;
}

// ---- per slab: a run handle (neighbour table, numbering, set-up) ----
int fvb_spatial_multi::open_slabs(bool try_fast)
{
    auto open_slab = [&](int r) -> int {
        SlabRun &sl = *slabs[r];
        FVB_HIP_CHECK(hipSetDevice(sl.dev));
        delete sl.run;
        sl.run = nullptr;
        if (sl.staged.dout.free_energy)
            FVB_HIP_CHECK(hipMemsetAsync(sl.staged.dout.free_energy, 0xff, sizeof(double) * (size_t)(sl.g1 - sl.g0), sl.stream)); // NaN (see fabber_vb_run_spatial_host)
        sl.run = new fvb_spatial_run;
        sl.run->allow_fast = sl.run->multi_fast = try_fast;
        sl.run->device_share = (int)std::count(devs.begin(), devs.begin() + world, sl.dev);
        return sl.run->open(&sl.staged.d, &sl.sp, sl.staged.b_data.p, &sl.staged.dout, sl.stream);
    };
    return for_each_slab(open_slab);
}

// a_K: every slab's segment sums, added in the order of the voxel list (vb_spatial_ak_reduce_kernel's), to every slab
int fvb_spatial_multi::reduce_ak()
{
    int rc;
    std::vector<double> partials, sums((size_t)P * 2, 0.0);
    for (int r = 0; r < world; r++)
    {
        SlabRun &sl = *slabs[r];
        FVB_HIP_CHECK(hipSetDevice(sl.dev));
        partials.assign((size_t)std::max(sl.run->n_segments, 1) * P * 2, 0.0);
        if ((rc = sl.run->ak_segment_sums(partials.data())) != 0)
            return rc;
        for (int seg = 0; seg < sl.run->n_segments; seg++)
            for (int j = 0; j < 2 * P; j++)
                sums[j] = sums[j] + partials[(size_t)seg * 2 * P + j];
    }
    for (int r = 0; r < world; r++)
    {
        FVB_HIP_CHECK(hipSetDevice(slabs[r]->dev));
        if ((rc = slabs[r]->run->set_ak_sums(sums.data())) != 0)
            return rc;
    }
    return 0;
}

// the F term of the priors of the LAST voxel of the sweep is the last slab's (inference_vb.cc:612,689,702)
int fvb_spatial_multi::hand_down_fprior()
{
    int rc;
    double fp = 0;
    FVB_HIP_CHECK(hipSetDevice(slabs[world - 1]->dev));
    if ((rc = fabber_vb_spatial_fprior(slabs[world - 1]->run, &fp, 0)) != 0)
        return rc;
    for (int r = 0; r + 1 < world; r++)
    {
        FVB_HIP_CHECK(hipSetDevice(slabs[r]->dev));
        if ((rc = fabber_vb_spatial_fprior(slabs[r]->run, &fp, 1)) != 0)
            return rc;
    }
    return 0;
}

// boundary planes both ways (the ghosts' means for the next iteration)
int fvb_spatial_multi::exchange_boundaries()
{
    int rc;
    for (int r = 0; r + 1 < world; r++)
    {
        SlabRun &lo = *slabs[r], &hi = *slabs[r + 1];
        const int up_from = std::max(lo.b, hi.g0);
        if ((rc = slab_transfer(lo, up_from - lo.g0, hi, up_from - hi.g0, lo.e - up_from, P)) != 0)
            return rc;
        const int down_to = std::min(hi.e, lo.g1);
        if ((rc = slab_transfer(hi, hi.b - hi.g0, lo, hi.b - lo.g0, down_to - hi.b, P)) != 0)
            return rc;
    }
    return 0;
}

// every slab's top plane writes into the inboxes of the slab above: peer access and the inbox addresses.
// Returns 1 where the devices turn out not to reach each other.
int fvb_spatial_multi::link_slabs()
{
    int rc;
    for (int r = 0; r + 1 < world; r++)
    {
        FVB_HIP_CHECK(hipSetDevice(slabs[r]->dev));
        if (slabs[r]->dev != slabs[r + 1]->dev)
        {
            hipError_t e = hipDeviceEnablePeerAccess(slabs[r + 1]->dev, 0);
            (void)hipGetLastError();
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
            {
                // (hipDeviceCanAccessPeer said yes: all the same, the pipeline needs no peer mapping)
                if (env.verbose)
                    fprintf(stderr, "[fvb spatial] hipDeviceEnablePeerAccess(%d -> %d): %s - level-chunk pipeline\n", slabs[r]->dev, slabs[r + 1]->dev, hipGetErrorString(e));
                return 1;
            }
        }
        if (r == s_unlink_pair) // (test hook: the slab above never hears from this one)
            continue;
        if ((rc = slabs[r]->run->link_up(*slabs[r + 1]->run, slabs[r]->g0, slabs[r + 1]->g0)) != 0)
            return rc;
    }
    return 0;
}

// ---- all slabs sweep together (the slab form of the split sweep on every slab). Returns 1 where that is given up. ----
int fvb_spatial_multi::sweep_together(void (*progress_cb)(int, int))
{
    int rc;
    if ((rc = link_slabs()) != 0)
        return rc;
    for (int it = 0; it < cfg.max_iterations; it++)
    {
        if (progress_cb)
            progress_cb(it, cfg.max_iterations); // inference_vb.cc:610
        if (has_spatial && (it > 0 || sp.update_first_iter) && (rc = reduce_ak()) != 0)
            return rc;
        // records of every slab, then ALL slabs' ordered sweeps at once (slab r + 1's lowest plane waits, voxel by
        // voxel, for what slab r's highest plane puts into its inboxes), then the second sweep
        for (int r = 0; r < world; r++)
        {
            FVB_HIP_CHECK(hipSetDevice(slabs[r]->dev));
            if ((rc = slabs[r]->run->fast_prep(it)) != 0)
                return rc;
        }
        for (int r = 0; r < world; r++)
        {
            FVB_HIP_CHECK(hipSetDevice(slabs[r]->dev));
            if ((rc = slabs[r]->run->fast_sweep()) != 0)
                return rc;
        }
        if (cfg.need_f && (rc = hand_down_fprior()) != 0)
            return rc;
        for (int r = 0; r < world; r++)
        {
            FVB_HIP_CHECK(hipSetDevice(slabs[r]->dev));
            if ((rc = slabs[r]->run->fast_noise(it)) != 0)
                return rc;
        }
        if (has_spatial && (rc = exchange_boundaries()) != 0)
            return rc;
    }
    bool any_failed = false;
    for (int r = 0; r < world; r++)
    {
        bool failed = false;
        FVB_HIP_CHECK(hipSetDevice(slabs[r]->dev));
        if ((rc = slabs[r]->run->fast_failed(failed)) != 0)
            return rc;
        any_failed |= failed;
    }
    if (any_failed)
    {
        // a voxel failed during a first sweep (or an inbox never arrived): as on one device, the run is repeated
        // with the launches the split sweep does not need - here the level-chunk pipeline
        if (env.verbose)
            fprintf(stderr, "[fvb spatial] slab sweep across devices abandoned, repeating the run with the level-chunk pipeline\n");
        return 1;
    }
    return 0;
}

// ---- the level-chunk pipeline: the global level range cut into chunks, slab r sweeps chunk c at tick c + r ----
int fvb_spatial_multi::sweep_pipeline(void (*progress_cb)(int, int))
{
    int rc;
    const int32_t *X = coords.data(), *Y = X + V, *Z = X + 2 * (size_t)V;
    const long long w0 = slabs[0]->run->level_w[0], w1 = slabs[0]->run->level_w[1], w2 = slabs[0]->run->level_w[2];
    long long lmin = LLONG_MAX, lmax = LLONG_MIN;
    for (int v = 0; v < V; v++)
    {
        const long long l = w0 * X[v] + w1 * Y[v] + w2 * Z[v];
        lmin = std::min(lmin, l);
        lmax = std::max(lmax, l);
    }
    long long chunk_levels = 16;
    if (env.chunk_levels.set) // tests: other cuts of the level range
        chunk_levels = std::max(1, env.chunk_levels.value);
    const long long nchunks = std::max(1LL, (lmax - lmin + chunk_levels) / chunk_levels);
    for (int it = 0; it < cfg.max_iterations; it++)
    {
        if (progress_cb)
            progress_cb(it, cfg.max_iterations); // inference_vb.cc:610
        if (has_spatial && (it > 0 || sp.update_first_iter) && (rc = reduce_ak()) != 0)
            return rc;
        for (long long tick = 0; tick < nchunks + world - 1; tick++)
        {
            for (int r = 0; r < world; r++)
            {
                const long long c = tick - r;
                if (c < 0 || c >= nchunks)
                    continue;
                FVB_HIP_CHECK(hipSetDevice(slabs[r]->dev));
                if ((rc = slabs[r]->run->sweep_levels(it, lmin + c * chunk_levels, lmin + (c + 1) * chunk_levels)) != 0)
                    return rc;
            }
            if (!has_spatial)
                continue;
            for (int r = 0; r + 1 < world; r++) // whoever swept hands its top planes up
            {
                const long long c = tick - r;
                if (c < 0 || c >= nchunks)
                    continue;
                SlabRun &lo = *slabs[r], &hi = *slabs[r + 1];
                const int from = std::max(lo.b, hi.g0);
                if ((rc = slab_transfer(lo, from - lo.g0, hi, from - hi.g0, lo.e - from, P)) != 0)
                    return rc;
            }
        }
        if (cfg.need_f && (rc = hand_down_fprior()) != 0)
            return rc;
        for (int r = 0; r < world; r++)
        {
            FVB_HIP_CHECK(hipSetDevice(slabs[r]->dev));
            if ((rc = slabs[r]->run->sweep_noise(it)) != 0)
                return rc;
        }
        if (has_spatial && (rc = exchange_boundaries()) != 0)
            return rc;
    }
    return 0;
}

// ---- results: the owned voxels of every slab go to the caller's images ----
int fvb_spatial_multi::download(const fvb_outputs *out)
{
    for (int r = 0; r < world; r++)
    {
        SlabRun &sl = *slabs[r];
        FVB_HIP_CHECK(hipSetDevice(sl.dev));
        const int rc = sl.staged.stage_out(out, sl.stream, nullptr, (size_t)(sl.b - sl.g0), (size_t)(sl.e - sl.b));
        if (rc)
            return rc;
    }
    return 0;
}

extern "C" {

static int32_t spatial_multi_validate(const fvb_config *cfg, const fvb_spatial *sp, const fvb_outputs *out)
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
    if (cfg->model == FVB_MODEL_HOSTJAC)
        return api_fail(-56, "a model evaluated on the host runs spatial VB on one device (fabber_vb_run_spatial_hostmodel_host)");
    if (cfg->model == FVB_MODEL_PLUGIN) // (a library's body exists as voxelwise wave kernels only: as the one-device entry point answers)
        return api_fail(-40, "no spatial kernel instantiation for this model / parameter count / noise model");
    if (!out || !out->mvn)
        return api_fail(-20, "outputs.mvn is required");
    return 0;
}

int32_t fabber_vb_spatial_multi_open(const fvb_config *cfg, const fvb_spatial *sp, const void *data, const fvb_outputs *wanted,
    const int32_t *devices, int32_t n_devices, fvb_spatial_multi **handle)
{
    if (!handle)
        return api_fail(-47, "handle pointer is NULL");
    *handle = nullptr;
    int rc = spatial_multi_validate(cfg, sp, wanted);
    if (rc)
        return rc;
    if (cfg->n_voxels == 0 || !data)
        return api_fail(-21, "no voxels / data is NULL");
    if (sp->locked_centres)
        return api_fail(-57, "locked linearisation centres run on one device (fabber_vb_run_spatial_host)");
    std::unique_ptr<fvb_spatial_multi> m(new fvb_spatial_multi);
    if ((rc = m->plan(cfg, sp, devices, n_devices)) != 0)
        return rc;
    if (m->world <= 1)
        return api_fail(-58, "the volume has too few planes for two slabs: fabber_vb_run_spatial_host / _device");
    if ((rc = m->upload(data, wanted)) != 0)
        return rc;
    *handle = m.release();
    return 0;
}

int32_t fabber_vb_spatial_multi_run(fvb_spatial_multi *handle, void (*progress_cb)(int, int))
{
    return handle ? handle->run(progress_cb) : api_fail(-47, "handle is NULL");
}

int32_t fabber_vb_spatial_multi_results(fvb_spatial_multi *handle, const fvb_outputs *out)
{
    if (!handle || !out || !out->mvn)
        return api_fail(-47, "handle or outputs.mvn is NULL");
    return handle->download(out);
}

int32_t fabber_vb_spatial_multi_slabs(fvb_spatial_multi *handle, int32_t *n_slabs, char *route, int32_t route_len)
{
    if (!handle)
        return api_fail(-47, "handle is NULL");
    if (n_slabs)
        *n_slabs = handle->world;
    if (route && route_len > 0)
        snprintf(route, (size_t)route_len, "%s", handle->route);
    return 0;
}

int32_t fabber_vb_spatial_multi_close(fvb_spatial_multi *handle)
{
    delete handle;
    return 0;
}

int32_t fabber_vb_run_spatial_host_multi(const fvb_config *cfg, const fvb_spatial *sp, const void *data, const fvb_outputs *out,
    const int32_t *devices, int32_t n_devices, void (*progress_cb)(int, int))
{
    const auto t0 = std::chrono::steady_clock::now();
    int rc = spatial_multi_validate(cfg, sp, out);
    if (rc)
        return rc;
    if (cfg->n_voxels == 0)
        return 0;
    if (!data)
        return api_fail(-21, "data is NULL");
    std::unique_ptr<fvb_spatial_multi> m(new fvb_spatial_multi);
    if ((rc = m->plan(cfg, sp, devices, n_devices)) != 0)
        return rc;
    // (locked centres: rare, and nothing a second device would speed up; too few planes for two slabs: the one-device run)
    if (sp->locked_centres || m->world <= 1)
        return fabber_vb_run_spatial_host(cfg, sp, data, out, m->devs[0], progress_cb);
    if ((rc = m->upload(data, out)) != 0)
        return rc;
    const double ms_up = ms_since(t0);
    if ((rc = m->run(progress_cb)) != 0)
        return rc;
    const auto t_out = std::chrono::steady_clock::now();
    if ((rc = m->download(out)) != 0)
        return rc;
    const double ms_out = ms_since(t_out);
    const auto t_free = std::chrono::steady_clock::now();
    m.reset();
    if (getenv("FVB_SPATIAL_TIMING"))
        fprintf(stderr, "[fvb spatial] fabber_vb_run_spatial_host_multi: upload %.1f ms, results %.1f ms, giving the slabs' memory back %.1f ms, %.1f ms in all\n",
            ms_up, ms_out, ms_since(t_free), ms_since(t0));
    return 0;
}

} // extern "C"
