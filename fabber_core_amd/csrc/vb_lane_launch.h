/*
 * vb_lane_launch.h - which of a model's lane-per-voxel kernels (vb_dispatch.h: LaneKernelInfo) a run takes, and their
 * launch. Shared by the engine (vb_api.hip: the built-in models) and by model libraries, whose kernels live in their own
 * code object (include/fabber_device_lane_model.h).
 */
#pragma once

#include "vb_dispatch.h"

#include <hip/hip_runtime.h>

#include <string>

namespace fvb
{
// how the series reaches the kernel (fvb_device_lane_launch_fn's `feed`)
enum LaneFeed
{
    LANE_FEED_STRIDED = 0,   // the caller's [t][voxel] image in place
    LANE_FEED_TILES_F32 = 1, // the tiled series, float
    LANE_FEED_TILES_F64 = 2  // the tiled series, double
};

// counting: the run's detector only counts iterations (convergence = maxits); the kernels built for that exist for the
// tile feeds with F, everything else takes the general kernel of its feed. NULL: the model has no kernel for the feed.
inline LaneKernelFn lane_kernel_fn(const LaneKernelInfo &k, int feed, bool counting)
{
    switch (feed)
    {
    case LANE_FEED_STRIDED:
        return k.fn;
    case LANE_FEED_TILES_F32:
        return (counting && k.fn_tiles_f32_counting) ? k.fn_tiles_f32_counting : k.fn_tiles_f32;
    case LANE_FEED_TILES_F64:
        return (counting && k.fn_tiles_f64_counting) ? k.fn_tiles_f64_counting : k.fn_tiles_f64;
    default:
        return nullptr;
    }
}

// One lane per voxel, 64-lane workgroups; the last wavefront is filled up by the kernel itself. lds: dynamic LDS (the
// several-precisions kernels' class bytes). The launch is asynchronous on `stream`.
inline int launch_lane_kernel(const LaneKernelInfo &k, const KernelArgs &ka, int feed, bool counting, size_t lds, hipStream_t stream,
    std::string &err)
{
    const LaneKernelFn fn = lane_kernel_fn(k, feed, counting);
    if (!fn)
    {
        err = std::string("lane kernel ") + (k.name ? k.name : "(none)") + ": no instantiation for feed " + std::to_string(feed);
        return -40;
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)((ka.cfg.n_voxels + 63) / 64)), dim3(64), lds, stream, ka);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
    {
        err = std::string("vb_lane_kernel launch: ") + hipGetErrorString(e);
        return -100 - (int)e;
    }
    return 0;
}
} // namespace fvb
