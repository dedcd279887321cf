/*
 * vb_wave_launch.h - launch of the wave-per-voxel kernels (vb_wave_kernel.h, vb_wave_ar_kernel.h) for one evaluator:
 * which of the family's kernels a configuration takes, the LDS attribute above 64 KB, one workgroup per voxel.
 * Shared by the engine (vb_wave.hip: the built-in evaluator) and by model libraries, whose kernels live in their own
 * code object (include/fabber_device_model.h).
 */
#pragma once

#include "vb_wave_ar_kernel.h"

#include <hip/hip_runtime.h>

#include <string>

namespace fvb
{
typedef void (*WaveKernelFn)(const KernelArgs, const WaveLayout);

// the kernels of one evaluator, [need_f]
struct WaveKernelSet
{
    WaveKernelFn white[2];
    WaveKernelFn ar_1_2[2], ar_2_2[2], ar_2_3[2], ar_2_4[2]; // AR(1): (echoes, alphas) - the alpha posterior lives in registers
};

template <class Eval>
WaveKernelSet wave_model_kernels()
{
    return WaveKernelSet{ { vb_wave_model_kernel<Eval, false>, vb_wave_model_kernel<Eval, true> },
        { vb_wave_ar_model_kernel<Eval, 1, 2, false>, vb_wave_ar_model_kernel<Eval, 1, 2, true> },
        { vb_wave_ar_model_kernel<Eval, 2, 2, false>, vb_wave_ar_model_kernel<Eval, 2, 2, true> },
        { vb_wave_ar_model_kernel<Eval, 2, 3, false>, vb_wave_ar_model_kernel<Eval, 2, 3, true> },
        { vb_wave_ar_model_kernel<Eval, 2, 4, false>, vb_wave_ar_model_kernel<Eval, 2, 4, true> } };
}

constexpr size_t WAVE_LDS_PER_WORKGROUP_MAX = 160 * 1024; // gfx950: 160 KB per CU, all of it addressable by one workgroup
constexpr size_t WAVE_LDS_DEFAULT_LIMIT = 64 * 1024;      // above this the kernel attribute has to be raised

inline int launch_wave_set(const WaveKernelSet &set, const KernelArgs &ka, hipStream_t stream, std::string &err)
{
    const fvb_config &cfg = ka.cfg;
    const bool ar = cfg.noise == FVB_NOISE_AR1;
    const WaveLayout L = wave_layout(cfg.n_times, cfg.n_params, cfg.n_phis, ar);
    if (L.bytes > WAVE_LDS_PER_WORKGROUP_MAX)
    {
        err = "wave kernel: " + std::to_string(L.bytes) + " bytes of LDS needed for T=" + std::to_string(cfg.n_times)
            + ", P=" + std::to_string(cfg.n_params) + " exceed the 160 KB of a gfx950 CU";
        return -41;
    }
    const int f = cfg.need_f ? 1 : 0;
    WaveKernelFn fn = set.white[f];
    if (ar) // one kernel per (echoes, alphas)
    {
        const int key = cfg.n_phis * 10 + 2 + cfg.ar_cross_terms;
        switch (key)
        {
        case 12:
            fn = set.ar_1_2[f];
            break;
        case 22:
            fn = set.ar_2_2[f];
            break;
        case 23:
            fn = set.ar_2_3[f];
            break;
        case 24:
            fn = set.ar_2_4[f];
            break;
        default:
            err = "AR(1) noise: num-echoes must be 1 or 2, cross terms need two echoes";
            return -40;
        }
    }
    if (L.bytes > WAVE_LDS_DEFAULT_LIMIT)
    {
        hipError_t e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.bytes);
        if (e != hipSuccess)
        {
            err = std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e);
            return -100 - (int)e;
        }
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)cfg.n_voxels), dim3(64), L.bytes, stream, ka, L);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
    {
        err = std::string("vb_wave_kernel launch: ") + hipGetErrorString(e);
        return -100 - (int)e;
    }
    return 0;
}
} // namespace fvb
