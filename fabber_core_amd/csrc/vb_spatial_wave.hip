// Spatial-VB kernels of the wave-per-voxel family (vb_spatial_wave.h): host-evaluated models, runtime parameter count
#include "vb_spatial_wave.h"

namespace fvb
{
SpatialKernels get_spatial_kernels_wide(int P, bool need_f)
{
    if (P < 1 || P > FVB_MAX_PARAMS)
        return SpatialKernels{};
    SpatialKernels k{};
    k.setup = vb_spatial_wave_setup_kernel;
    k.ak_partial = vb_spatial_wide_ak_partial_kernel;
    k.ak_reduce = vb_spatial_wide_ak_reduce_kernel;
    k.ak_final = vb_spatial_wide_ak_final_kernel;
    k.theta = need_f ? (SpatialThetaFn)vb_spatial_wave_theta_kernel<true> : (SpatialThetaFn)vb_spatial_wave_theta_kernel<false>;
    k.noise = need_f ? (SpatialKernelFn)vb_spatial_wave_noise_kernel<true> : (SpatialKernelFn)vb_spatial_wave_noise_kernel<false>;
    k.pack = vb_spatial_wide_pack_kernel;
    k.state_rows = sp_wide_layout(P).ROWS;
    k.name = "spatial<host,wave>";
    // (no split first sweep: prep, noise_fast and slab_sweep stay NULL - a host model's means must be complete on the
    // host before the second sweep starts)
    k.wave = 1;
    k.wave_lds = sp_wave_layout(P).bytes;
    return k;
}
} // namespace fvb
