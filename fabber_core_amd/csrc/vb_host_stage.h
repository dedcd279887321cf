/*
 * vb_host_stage.h - what the entry points that take HOST pointers share (vb_api.hip, vb_spatial_api.hip,
 * vb_spatial_multi.hip, vb_hostmodel_api.hip, vb_nlls.hip): the error macro and the helpers of vb_api.hip, the device
 * buffer type, the parameter table on the device, a problem's inputs and outputs on the device (StagedProblem) and the
 * loop of the routes whose forward model is evaluated by the caller (HostModelLoop). No kernel includes this file.
 */
#pragma once

#include "../../include/fabber_vb.h"
#include "vb_host_copy.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace fvb
{
// vb_api.hip
int api_fail(int code, const std::string &msg);
int api_validate(const fvb_config *cfg, bool allow_spatial);
int api_variant(); // fabber_vb_set_variant: 0 auto, 1 lane, 2 wave
int api_residual_mode();
int api_precise_passes();
double api_residual_tol();
void api_keep_pool_memory();
hipError_t api_pool_alloc(void **p, size_t bytes, hipStream_t stream);
hipError_t api_pool_free(void *p, hipStream_t stream);
hipError_t api_take_side_stream(hipStream_t *out, int *device);
void api_return_side_stream(hipStream_t s, int device);

#define FVB_HIP_CHECK(expr)                                                                                  \
    do                                                                                                       \
    {                                                                                                        \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fvb::api_fail(-100 - (int)e_, std::string(#expr) + ": " + hipGetErrorString(e_));         \
    } while (0)

// timepoints that take part in the fit (phi_index, host memory: 255 = masked; NULL = all of them)
inline int count_unmasked(size_t T, const uint8_t *phi_index)
{
    if (!phi_index)
        return (int)T;
    int n = 0;
    for (size_t t = 0; t < T; t++)
        n += (phi_index[t] != 255);
    return n;
}

// entries of the noise block of the result MVN (WhiteParams / Ar1cParams::OutputAsMVN; AR(1): alphas and phi means,
// noisemodel_ar.cc:287-300)
inline int noise_outputs(const fvb_config *cfg)
{
    return cfg->noise == FVB_NOISE_WHITE ? cfg->n_phis : 2 + cfg->ar_cross_terms + cfg->n_phis;
}

// Device memory of ONE block of the pipelined host entry point: plain hipMalloc'd buffers that stay with the call's cached
// streams (PipeStreams) and are handed out again - to the block that takes the slot three blocks later, and to the next
// call. No stream-ordered pool here: upload, fit and download streams and two host threads work on a call, and with ROCm
// 7.2's runtime buffers taken from ONE pool by several streams came out overlapping - wrong results from the pipelined
// call, right ones with plain hipMalloc in the same code (tools/measure/runtime_check.py, runtime_check_capi.py); ROCm 7.0's
// runtime did not show it. A slot's buffers are reused only after the block that had them has been SEEN to finish.
struct BlockSlot
{
    struct Buf
    {
        void *p;
        size_t cap;
        bool used;
    };
    std::vector<Buf> bufs;
    hipError_t take(void **out, size_t bytes)
    {
        int best = -1;
        for (size_t i = 0; i < bufs.size(); i++)
            if (!bufs[i].used && bufs[i].cap >= bytes && (best < 0 || bufs[i].cap < bufs[(size_t)best].cap))
                best = (int)i;
        if (best < 0)
        {
            const size_t cap = (bytes + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
            void *p = nullptr;
            const hipError_t e = hipMalloc(&p, cap);
            if (e != hipSuccess)
                return e;
            bufs.push_back(Buf{ p, cap, false });
            best = (int)bufs.size() - 1;
        }
        bufs[(size_t)best].used = true;
        *out = bufs[(size_t)best].p;
        return hipSuccess;
    }
    void reset()
    {
        for (Buf &b : bufs)
            b.used = false;
    }
    void destroy()
    {
        for (Buf &b : bufs)
            (void)hipFree(b.p);
        bufs.clear();
    }
};

// Where a DevMem takes its memory from. The pool is the library's stream-ordered one (api_pool_alloc): it keeps what a
// run gives back, so a caller that runs volume after volume pays for its allocations once (hipMalloc + hipFree of the
// series-sized buffers were ~20 of the 50 ms a call on 1e6 voxels took through host pointers; 4 ms per spatial run of
// 128^3 voxels).
struct MemSource
{
    bool plain = false;        // hipMalloc / hipFree
    BlockSlot *slot = nullptr; // borrowed from the slot (nothing to free)
};
inline MemSource from_pool()
{
    return MemSource();
}
inline MemSource from_malloc()
{
    return MemSource{ true, nullptr };
}
inline MemSource from_slot(BlockSlot *slot)
{
    return slot ? MemSource{ false, slot } : MemSource();
}

// RAII device buffer of the host entry points and the spatial driver
struct DevMem
{
    void *p = nullptr;
    hipStream_t stream = nullptr; // pool memory: allocated and freed in this stream's order
    bool plain = false;           // hipMalloc'ed, not from the pool
    bool fine = false;            // ... and really fine-grained (alloc_fine falls back to ordinary device memory)
    bool borrowed = false;        // a BlockSlot's
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem()
    {
        reset();
    }
    void reset()
    {
        if (p && plain)
            (void)hipFree(p);
        else if (p && !borrowed)
            (void)api_pool_free(p, stream);
        p = nullptr;
        plain = fine = borrowed = false;
    }
    hipError_t alloc(size_t bytes, hipStream_t s = nullptr, MemSource src = MemSource())
    {
        bytes = bytes ? bytes : 8;
        stream = s;
        plain = src.plain;
        borrowed = src.slot != nullptr;
        if (src.slot)
            return src.slot->take(&p, bytes);
        return plain ? hipMalloc(&p, bytes) : api_pool_alloc(&p, bytes, s);
    }
    // memory that a kernel on ANOTHER device writes while a kernel on this one polls it (the inboxes of the slab sweep
    // across devices): fine-grained, i.e. not held in this device's L2 between the polls
    hipError_t alloc_fine(size_t bytes)
    {
        plain = true;
        hipError_t e = hipExtMallocWithFlags(&p, bytes ? bytes : 8, hipDeviceMallocFinegrained);
        fine = (e == hipSuccess);
        if (e != hipSuccess)
        {
            // ordinary device memory: good for slabs that share a device; across devices a remote store might stay
            // invisible to the polling device's L2, so the caller takes the level-chunk pipeline then (gran_fine)
            (void)hipGetLastError();
            e = hipMalloc(&p, bytes ? bytes : 8);
        }
        return e;
    }
};

// a buffer for `bytes` of host memory and their copy into it, enqueued on `stream`
inline int upload_array(DevMem &b, const void *host, size_t bytes, hipStream_t stream, MemSource src = MemSource())
{
    FVB_HIP_CHECK(b.alloc(bytes, stream, src));
    FVB_HIP_CHECK(hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, stream));
    return 0;
}

// A host fvb_param_table (fvb_config.params_ext: more than FVB_MAX_PARAMS parameters) on the device: the seven arrays,
// the image priors of the voxels [v0, v0 + Vb) and the table itself.
// priors = false (method=nlls: the minimiser reads the transforms and the starting estimate, the prior entries are
// carried for the post-processing kernel): arrays may be NULL, prior types are not looked at, no images go up.
struct DeviceParamTable
{
    DevMem block;
    std::vector<std::unique_ptr<DevMem> > images;
    const fvb_param_table *device = nullptr;
    int upload(const fvb_config *cfg, size_t v0, size_t Vb, hipStream_t stream, MemSource src = MemSource(), bool priors = true)
    {
        const fvb_param_table *h = cfg->params_ext;
        const size_t P = (size_t)cfg->n_params;
        // [table][transform, prior_type: int32 P each][5 double arrays][image pointers]
        const size_t off_i = sizeof(fvb_param_table), off_d = off_i + 2 * P * sizeof(int32_t) + (2 * P * sizeof(int32_t)) % 8;
        const size_t off_p = off_d + 5 * P * sizeof(double), bytes = off_p + P * sizeof(double *);
        std::vector<char> host(bytes, 0);
        FVB_HIP_CHECK(block.alloc(bytes, stream, src));
        char *dev = (char *)block.p;
        fvb_param_table t;
        t.transform = (const int32_t *)(dev + off_i);
        t.prior_type = t.transform + P;
        t.prior_mean = (const double *)(dev + off_d);
        t.prior_var = t.prior_mean + P;
        t.prior_prec = t.prior_var + P;
        t.post_mean = t.prior_prec + P;
        t.post_var = t.post_mean + P;
        t.image_prior = (const double *const *)(dev + off_p);
        memcpy(host.data(), &t, sizeof(t));
        memcpy(host.data() + off_i, h->transform, P * sizeof(int32_t));
        if (priors || h->prior_type)
            memcpy(host.data() + off_i + P * sizeof(int32_t), h->prior_type, P * sizeof(int32_t));
        const double *arrays[5] = { h->prior_mean, h->prior_var, h->prior_prec, h->post_mean, h->post_var };
        for (int a = 0; a < 5; a++)
            if (priors || arrays[a])
                memcpy(host.data() + off_d + (size_t)a * P * sizeof(double), arrays[a], P * sizeof(double));
        const double **img = (const double **)(host.data() + off_p);
        for (size_t k = 0; k < P && priors; k++)
        {
            if (h->prior_type[k] < 0 || h->prior_type[k] > FVB_PRIOR_ARD)
                return api_fail(-14, "a parameter table takes prior types N, I and ARD");
            if (h->prior_type[k] == FVB_PRIOR_IMAGE && !(h->image_prior && h->image_prior[k]))
                return api_fail(-13, "image prior without an image");
            if (h->image_prior && h->image_prior[k])
            {
                images.emplace_back(new DevMem);
                FVB_HIP_CHECK(images.back()->alloc(sizeof(double) * Vb, stream, src));
                FVB_HIP_CHECK(hipMemcpyAsync(images.back()->p, h->image_prior[k] + v0, sizeof(double) * Vb, hipMemcpyHostToDevice, stream));
                img[k] = (const double *)images.back()->p;
            }
        }
        FVB_HIP_CHECK(hipMemcpyAsync(block.p, host.data(), bytes, hipMemcpyHostToDevice, stream));
        FVB_HIP_CHECK(hipStreamSynchronize(stream)); // (`host` is a local; the image priors are the caller's pageable memory)
        device = (const fvb_param_table *)block.p;
        return 0;
    }
};

// Voxels [v0, v1) of a problem given through HOST pointers, on the current device: the range's columns of every
// [row][voxel] image go up and down as 2-D copies (row pitch = the caller's n_voxels; one contiguous copy where the
// range is the whole volume), `d` and `dout` describe a problem of v1 - v0 voxels in device memory. Everything is
// enqueued on the caller's stream; nothing here waits, but for the parameter table's upload and the end of stage_out.
enum StageParts : unsigned
{
    STAGE_INIT_MVN = 1, // cfg->init_mvn
    STAGE_PRIORS = 2,   // the image priors; the parameter table with its prior entries checked
    STAGE_HISTORY = 4,  // outputs f_history (NaN-filled in the stream) and f_history_len
    STAGE_VB = STAGE_INIT_MVN | STAGE_PRIORS | STAGE_HISTORY,
    STAGE_SPATIAL = STAGE_INIT_MVN | STAGE_PRIORS,
    STAGE_NLLS = 0
};
struct StagedProblem
{
    fvb_config d;
    fvb_outputs dout;
    size_t V = 0, v0 = 0, Vb = 0, mvn_rows = 0, history_rows = 0;
    DevMem b_data, b_design, b_consts, b_supp, b_phi, b_init, b_img[FVB_MAX_PARAMS], b_mvn, b_small, b_hist;
    // F (8 bytes), history length, status, iterations (4 each) of a voxel: one device buffer, [F][hlen][status][it]
    static constexpr size_t SMALL_BYTES_PER_VOXEL = 8 + 4 + 4 + 4;
    size_t small_bytes = 0;
    DeviceParamTable ptable;

    // out: the sections the caller wants (only which pointers are set is looked at)
    int stage_in(const fvb_config *cfg, const void *data, const fvb_outputs *out, size_t rows, size_t v0_, size_t v1, hipStream_t stream,
        MemSource src, unsigned parts)
    {
        V = (size_t)cfg->n_voxels;
        v0 = v0_;
        Vb = v1 - v0;
        mvn_rows = rows;
        const size_t T = (size_t)cfg->n_times, P = (size_t)cfg->n_params, esz = cfg->data_f64 ? 8 : 4;
        auto upload = [&](DevMem &b, const void *host, size_t elem, size_t nrows) -> int {
            FVB_HIP_CHECK(b.alloc(nrows * Vb * elem, stream, src));
            FVB_HIP_CHECK(copy_rows(b.p, Vb * elem, (const char *)host + v0 * elem, V * elem, Vb * elem, nrows, hipMemcpyHostToDevice, stream));
            return 0;
        };
        int rc;
        d = *cfg;
        d.n_voxels = (int32_t)Vb;
        if ((rc = upload(b_data, data, esz, T)) != 0)
            return rc;
        if (cfg->design)
        {
            if ((rc = upload_array(b_design, cfg->design, sizeof(double) * T * P, stream, src)) != 0)
                return rc;
            d.design = (const double *)b_design.p;
        }
        if (cfg->model == FVB_MODEL_PLUGIN && cfg->model_consts && cfg->n_model_consts > 0) // a library model's constants
        {
            if ((rc = upload_array(b_consts, cfg->model_consts, sizeof(double) * (size_t)cfg->n_model_consts, stream, src)) != 0)
                return rc;
            d.model_consts = (const double *)b_consts.p;
        }
        d.model_supp = nullptr; // (a host pointer; only a library's body reads the device copy)
        if (cfg->model == FVB_MODEL_PLUGIN && cfg->model_supp && cfg->n_model_supp > 0) // its voxels' supplementary data:
        {                                                                               // the rows' columns [v0, v1)
            if ((rc = upload(b_supp, cfg->model_supp, sizeof(double), (size_t)cfg->n_model_supp)) != 0)
                return rc;
            d.model_supp = (const double *)b_supp.p;
        }
        if (cfg->phi_index)
        {
            if ((rc = upload_array(b_phi, cfg->phi_index, T, stream, src)) != 0)
                return rc;
            d.phi_index = (const uint8_t *)b_phi.p;
        }
        if (cfg->init_mvn && (parts & STAGE_INIT_MVN))
        {
            if ((rc = upload(b_init, cfg->init_mvn, sizeof(double), rows)) != 0)
                return rc;
            d.init_mvn = (const double *)b_init.p;
        }
        if (cfg->params_ext) // more than FVB_MAX_PARAMS parameters: the per-parameter entries as a table on the device
        {
            if ((rc = ptable.upload(cfg, v0, Vb, stream, src, (parts & STAGE_PRIORS) != 0)) != 0)
                return rc;
            d.params_ext = ptable.device;
        }
        for (size_t k = 0; k < P && !cfg->params_ext && (parts & STAGE_PRIORS); k++)
            if (cfg->image_prior[k])
            {
                if ((rc = upload(b_img[k], cfg->image_prior[k], sizeof(double), 1)) != 0)
                    return rc;
                d.image_prior[k] = (const double *)b_img[k].p;
            }
        memset(&dout, 0, sizeof(dout));
        FVB_HIP_CHECK(b_mvn.alloc(sizeof(double) * rows * Vb, stream, src));
        dout.mvn = (double *)b_mvn.p;
        {
            // (sections the caller does not want are left out; every section starts on a multiple of 8 bytes because F
            // comes first and the int sections are padded to an even number of voxels)
            const bool want_hlen = out->f_history_len && (parts & STAGE_HISTORY);
            const size_t ints = (Vb + 1) / 2 * 2 * sizeof(int32_t);
            small_bytes = (out->free_energy ? sizeof(double) * Vb : 0) + (want_hlen ? ints : 0) + (out->status ? ints : 0)
                + (out->iterations ? ints : 0);
            FVB_HIP_CHECK(b_small.alloc(small_bytes, stream, src));
            char *q = (char *)b_small.p;
            if (out->free_energy)
            {
                dout.free_energy = (double *)q;
                q += sizeof(double) * Vb;
            }
            if (want_hlen)
            {
                dout.f_history_len = (int32_t *)q;
                q += ints;
            }
            if (out->status)
            {
                dout.status = (int32_t *)q;
                q += ints;
            }
            if (out->iterations)
                dout.iterations = (int32_t *)q;
        }
        if (out->f_history && cfg->f_history_rows > 0 && (parts & STAGE_HISTORY))
        {
            history_rows = (size_t)cfg->f_history_rows;
            FVB_HIP_CHECK(b_hist.alloc(sizeof(double) * history_rows * Vb, stream, src));
            FVB_HIP_CHECK(hipMemsetAsync(b_hist.p, 0xff, sizeof(double) * history_rows * Vb, stream)); // NaN fill
            dout.f_history = (double *)b_hist.p;
        }
        return 0;
    }
    // The staged voxels [first, first + count) into the caller's images; returns after they have arrived.
    // bounce: pinned host memory of at least small_bytes (the small arrays come down in one copy and are handed out from
    // there; the whole range only), or NULL: one copy per array
    int stage_out(const fvb_outputs *out, hipStream_t stream, void *bounce = nullptr, size_t first = 0, size_t count = (size_t)-1)
    {
        count = std::min(count, Vb - first);
        auto download = [&](void *dst, const void *src, size_t elem, size_t nrows) {
            return copy_rows((char *)dst + (v0 + first) * elem, V * elem, (const char *)src + first * elem, Vb * elem, count * elem, nrows,
                hipMemcpyDeviceToHost, stream);
        };
        if (bounce && small_bytes)
            FVB_HIP_CHECK(hipMemcpyAsync(bounce, b_small.p, small_bytes, hipMemcpyDeviceToHost, stream)); // (ahead of the big one)
        FVB_HIP_CHECK(download(out->mvn, dout.mvn, sizeof(double), mvn_rows));
        if (dout.f_history && out->f_history)
            FVB_HIP_CHECK(download(out->f_history, dout.f_history, sizeof(double), history_rows));
        if (!bounce)
        {
            if (dout.free_energy && out->free_energy)
                FVB_HIP_CHECK(download(out->free_energy, dout.free_energy, sizeof(double), 1));
            if (dout.f_history_len && out->f_history_len)
                FVB_HIP_CHECK(download(out->f_history_len, dout.f_history_len, sizeof(int32_t), 1));
            if (dout.status && out->status)
                FVB_HIP_CHECK(download(out->status, dout.status, sizeof(int32_t), 1));
            if (dout.iterations && out->iterations)
                FVB_HIP_CHECK(download(out->iterations, dout.iterations, sizeof(int32_t), 1));
        }
        FVB_HIP_CHECK(hipStreamSynchronize(stream));
        if (bounce && small_bytes)
        {
            const char *base = (const char *)b_small.p;
            auto hand_out = [&](void *dst, const void *dev, size_t elem) {
                memcpy((char *)dst + v0 * elem, (const char *)bounce + ((const char *)dev - base), Vb * elem);
            };
            if (dout.free_energy)
                hand_out(out->free_energy, dout.free_energy, sizeof(double));
            if (dout.f_history_len)
                hand_out(out->f_history_len, dout.f_history_len, sizeof(int32_t));
            if (dout.status)
                hand_out(out->status, dout.status, sizeof(int32_t));
            if (dout.iterations)
                hand_out(out->iterations, dout.iterations, sizeof(int32_t));
        }
        return 0;
    }
    // (pool memory goes back in its stream's order: for an owner that destroys that stream itself)
    void release()
    {
        for (DevMem *m : { &b_data, &b_design, &b_consts, &b_supp, &b_phi, &b_init, &b_mvn, &b_small, &b_hist, &ptable.block })
            m->reset();
        for (DevMem &m : b_img)
            m.reset();
        ptable.images.clear();
    }
};

// The loop of the routes whose forward model exists only as host code (voxelwise VB and method=nlls): the caller's
// callback linearises the model about the current means of the voxels still running, one launch of a step kernel takes
// them one step on, until every voxel reports the done phase.
// The voxels still running are worked through in batches: the linearisations of a batch (g and J, T (P + 1) doubles per
// voxel) are what the host and the device hold at a time, in two buffers each side, so that the host evaluates the model
// for the next batch while the device steps the current one. (One buffer for the whole volume - 4 GB per million voxels
// at T = 100, P = 4 - made real volumes fail at allocation.)
struct HostModelLoop
{
    size_t V = 0, P = 0, lin_stride = 0, batch_voxels = 0;
    DevMem b_lin[2], b_ids[2], b_means, b_phase; // b_means [V][P], b_phase [V]: what the step kernel reports
    int open(const fvb_config *cfg)
    {
        V = (size_t)cfg->n_voxels;
        P = (size_t)cfg->n_params;
        lin_stride = (size_t)cfg->n_times * (P + 1);
        batch_voxels = std::max<size_t>(1, std::min<size_t>(V, std::max<size_t>(4096, (size_t)(256u << 20) / (sizeof(double) * lin_stride))));
        if (const char *forced = getenv("FVB_HOSTMODEL_BATCH")) // tests: several batches on small volumes
            batch_voxels = std::max<size_t>(1, std::min<size_t>(V, (size_t)atol(forced)));
        for (int i = 0; i < 2; i++)
        {
            FVB_HIP_CHECK(b_lin[i].alloc(sizeof(double) * lin_stride * batch_voxels, nullptr, from_malloc()));
            FVB_HIP_CHECK(b_ids[i].alloc(sizeof(int32_t) * batch_voxels, nullptr, from_malloc()));
        }
        FVB_HIP_CHECK(b_means.alloc(sizeof(double) * P * V, nullptr, from_malloc()));
        FVB_HIP_CHECK(b_phase.alloc(sizeof(int32_t) * V, nullptr, from_malloc()));
        return 0;
    }
    // means: [V][P] (Fabber space), the starting estimate. launch(lin, batch_ids, nb, stream) enqueues one step of the nb
    // voxels batch_ids[.] with their linearisations lin (device memory). not_terminated: the text of error -53.
    template <class Launch>
    int run(fvb_linearise_fn linearise, void *user, std::vector<double> &means, int done_phase, long max_steps, const char *not_terminated,
        Launch launch)
    {
        std::vector<double> lin[2], active_means;
        lin[0].resize(lin_stride * batch_voxels);
        lin[1].resize(lin_stride * batch_voxels);
        std::vector<int32_t> phase(V, 0), ids; // (phase 0: new)
        hipStream_t stream;
        FVB_HIP_CHECK(hipStreamCreate(&stream));
        struct StreamGuard
        {
            hipStream_t s;
            ~StreamGuard()
            {
                (void)hipStreamSynchronize(s);
                (void)hipStreamDestroy(s);
            }
        } stream_guard = { stream };
        hipEvent_t used[2]; // buffer pair i is free again when the launch that read it is over
        FVB_HIP_CHECK(hipEventCreateWithFlags(&used[0], hipEventDisableTiming));
        FVB_HIP_CHECK(hipEventCreateWithFlags(&used[1], hipEventDisableTiming));
        struct EventGuard
        {
            hipEvent_t *e;
            ~EventGuard()
            {
                (void)hipEventDestroy(e[0]);
                (void)hipEventDestroy(e[1]);
            }
        } event_guard = { used };
        for (long step = 0;; step++)
        {
            ids.clear();
            for (size_t v = 0; v < V; v++)
                if (phase[v] != done_phase)
                    ids.push_back((int32_t)v);
            if (ids.empty())
                break;
            if (step >= max_steps)
                return api_fail(-53, not_terminated);
            int which = 0;
            for (size_t b0 = 0; b0 < ids.size(); b0 += batch_voxels, which ^= 1)
            {
                const size_t nb = std::min(batch_voxels, ids.size() - b0);
                active_means.resize(nb * P);
                for (size_t a = 0; a < nb; a++)
                    for (size_t i = 0; i < P; i++)
                        active_means[a * P + i] = means[(size_t)ids[b0 + a] * P + i];
                // (the launch that read this host / device buffer pair two batches ago has to be over; the host
                // works on this batch's model evaluations while the device steps the previous batch)
                if (b0 >= 2 * batch_voxels)
                    FVB_HIP_CHECK(hipEventSynchronize(used[which]));
                // g [T] then J [T][P] per voxel of the batch, about active_means[a][.] (Fabber space)
                const int cb = linearise(user, (int32_t)nb, ids.data() + b0, active_means.data(), lin[which].data());
                if (cb != 0)
                    return api_fail(-54, "the model's linearisation callback failed (code " + std::to_string(cb) + ")");
                FVB_HIP_CHECK(hipMemcpyAsync(b_lin[which].p, lin[which].data(), sizeof(double) * lin_stride * nb, hipMemcpyHostToDevice, stream));
                FVB_HIP_CHECK(hipMemcpyAsync(b_ids[which].p, ids.data() + b0, sizeof(int32_t) * nb, hipMemcpyHostToDevice, stream));
                launch((const double *)b_lin[which].p, (const int32_t *)b_ids[which].p, nb, stream);
                FVB_HIP_CHECK(hipGetLastError());
                FVB_HIP_CHECK(hipEventRecord(used[which], stream));
            }
            FVB_HIP_CHECK(hipStreamSynchronize(stream));
            FVB_HIP_CHECK(hipMemcpy(phase.data(), b_phase.p, sizeof(int32_t) * V, hipMemcpyDeviceToHost));
            FVB_HIP_CHECK(hipMemcpy(means.data(), b_means.p, sizeof(double) * P * V, hipMemcpyDeviceToHost));
        }
        return 0;
    }
};
} // namespace fvb
