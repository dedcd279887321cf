/*
 * vb_nlls_launch.h - which of a model's NLLS minimisers (vb_nlls_kernel.h) a run takes, and their launch: one lane per
 * voxel in 64-lane workgroups, or one 64-lane workgroup per voxel with the LDS attribute raised above 64 KB.
 * Shared by the engine (vb_nlls.hip: the built-in models) and by model libraries, whose kernels live in their own code
 * object (include/fabber_device_nlls_model.h).
 */
#pragma once

#include "vb_nlls_kernel.h"
#include "vb_wave_launch.h"

#include <hip/hip_runtime.h>

#include <string>

namespace fvb
{
typedef void (*NllsWaveKernelFn)(const NllsArgs, const WaveLayout);

// the kernel variant a caller may force (fabber_vb_set_variant)
enum NllsVariant
{
    NLLS_VARIANT_AUTO = 0,
    NLLS_VARIANT_LANE = 1,
    NLLS_VARIANT_WAVE = 2
};

// from this many voxels on the lane-per-voxel minimiser fills the chip (measured for the built-in models)
constexpr int NLLS_LANE_MIN_VOXELS = 4096;

inline WaveLayout nlls_wave_layout(const fvb_config &cfg)
{
    return wave_layout(cfg.n_times, cfg.n_params, 1);
}

// Lane per voxel where the model has a lane minimiser for the parameter count and there are enough voxels to fill the
// chip (as the VB kernels) or the series does not fit the wave kernel's LDS; wave per voxel otherwise.
inline bool nlls_takes_lane(bool has_lane, int variant, const fvb_config &cfg)
{
    if (!has_lane || variant == NLLS_VARIANT_WAVE)
        return false;
    return variant == NLLS_VARIANT_LANE || cfg.n_voxels >= NLLS_LANE_MIN_VOXELS || nlls_wave_layout(cfg).bytes > WAVE_LDS_PER_WORKGROUP_MAX;
}

// lane / wave: the model's two minimisers, either may be NULL. The launch is asynchronous on `stream`.
inline int launch_nlls_kernel(NllsKernelFn lane, NllsWaveKernelFn wave, int variant, const NllsArgs &na, hipStream_t stream, std::string &err)
{
    const fvb_config &cfg = na.ka.cfg;
    if (cfg.n_voxels <= 0)
        return 0;
    if (nlls_takes_lane(lane != nullptr, variant, cfg))
        hipLaunchKernelGGL(lane, dim3((unsigned)((cfg.n_voxels + 63) / 64)), dim3(64), 0, stream, na);
    else
    {
        if (!wave)
        {
            err = "NLLS: no wave-per-voxel minimiser for this model";
            return -40;
        }
        const WaveLayout L = nlls_wave_layout(cfg);
        if (L.bytes > WAVE_LDS_PER_WORKGROUP_MAX)
        {
            err = "NLLS wave kernel: " + std::to_string(L.bytes) + " bytes of LDS needed for T=" + std::to_string(cfg.n_times)
                + ", P=" + std::to_string(cfg.n_params) + " exceed the 160 KB of a gfx950 CU";
            return -41;
        }
        if (L.bytes > WAVE_LDS_DEFAULT_LIMIT)
        {
            hipError_t e = hipFuncSetAttribute((const void *)wave, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.bytes);
            if (e != hipSuccess)
            {
                err = std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e);
                return -100 - (int)e;
            }
        }
        hipLaunchKernelGGL(wave, dim3((unsigned)cfg.n_voxels), dim3(64), L.bytes, stream, na, L);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
    {
        err = std::string("vb_nlls_kernel launch: ") + hipGetErrorString(e);
        return -100 - (int)e;
    }
    return 0;
}
} // namespace fvb
