// Wave-per-voxel kernel: launch (see vb_wave_kernel.h for the mapping, vb_wave_launch.h for the launch itself).
#include "vb_wave_launch.h"

namespace fvb
{
int launch_wave_kernel(const KernelArgs &ka, hipStream_t stream, std::string &err)
{
    const fvb_config &cfg = ka.cfg;
    if (cfg.model != FVB_MODEL_POLY && cfg.model != FVB_MODEL_LINEAR && cfg.model != FVB_MODEL_EXP)
    {
        err = "wave kernel: model has no device body";
        return -40;
    }
    static const WaveKernelSet builtin = { { vb_wave_kernel<false>, vb_wave_kernel<true> },
        { vb_wave_ar_kernel<1, 2, false>, vb_wave_ar_kernel<1, 2, true> }, { vb_wave_ar_kernel<2, 2, false>, vb_wave_ar_kernel<2, 2, true> },
        { vb_wave_ar_kernel<2, 3, false>, vb_wave_ar_kernel<2, 3, true> }, { vb_wave_ar_kernel<2, 4, false>, vb_wave_ar_kernel<2, 4, true> } };
    return launch_wave_set(builtin, ka, stream, err);
}
} // namespace fvb
