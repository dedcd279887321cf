// Spatial-VB kernels of the wave-per-voxel family (vb_spatial_wave.h): host-evaluated models, runtime parameter count
#define FVB_SPATIAL_WAVE_ENGINE 1 // (the family's kernels that are no templates are defined here, once)
#include "vb_spatial_wave_ar.h"

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

// The family around the device body of a model library (vb_spatial_wave_model.h,
// include/fabber_device_spatial_wave_model.h): the table above with the two kernels that read the linearisation left to
// the library's launcher and the LDS of the layout those kernels place their arrays in (the engine's first sweep uses
// the front of it: sp_wave_layout's offsets are that layout's).
SpatialKernels get_spatial_kernels_wave_model(int P, bool need_f)
{
    SpatialKernels k = get_spatial_kernels_wide(P, need_f);
    if (!k.theta)
        return k;
    k.setup = k.noise = nullptr; // the library's
    k.name = nullptr;
    k.wave_lds = sp_wave_model_layout(P).bytes;
    return k;
}
// ... and under a noise pattern of N = 2 ... FVB_MAX_PHIS precisions (include/fabber_device_spatial_wave_noise_model.h):
// the first sweep in its form for N classes, the state image with the class rows, the LDS of the layout for (P, N)
SpatialKernels get_spatial_kernels_wave_noise_model(int P, int N, bool need_f)
{
    SpatialKernels k = get_spatial_kernels_wave_model(P, need_f);
    if (!k.theta || N < 2 || N > FVB_MAX_PHIS)
        return SpatialKernels{};
    k.theta = need_f ? (SpatialThetaFn)vb_spatial_wave_theta_kernel<true, true> : (SpatialThetaFn)vb_spatial_wave_theta_kernel<false, true>;
    k.state_rows = sp_wide_state_rows(P, N);
    k.wave_lds = sp_wave_model_layout(P, N).bytes;
    return k;
}
uint32_t spatial_wave_noise_model_lds_probe()
{
    return (uint32_t)sp_wave_model_layout(FVB_MAX_PARAMS, FVB_MAX_PHIS).n_doubles;
}
// ... and under AR(1) noise with one echo and no cross terms (include/fabber_device_spatial_wave_ar_model.h): the first
// sweep with the AR free energy where F is evaluated (without F it is the one-precision kernel, on the effective moments),
// the state image with the rows of SpAr1, the LDS of the layout with the AR areas
SpatialKernels get_spatial_kernels_wave_ar_model(int P, bool need_f)
{
    SpatialKernels k = get_spatial_kernels_wave_model(P, need_f);
    if (!k.theta)
        return SpatialKernels{};
    if (need_f)
        k.theta = vb_spatial_wave_ar_theta_kernel;
    k.state_rows = sp_wide_ar_state_rows(P);
    k.wave_lds = sp_wave_ar_model_layout(P).bytes;
    return k;
}
uint32_t spatial_wave_ar_model_lds_probe()
{
    return (uint32_t)sp_wave_ar_model_layout(FVB_MAX_PARAMS).n_doubles;
}
// what a library's entry must report as its lds_probe and as its wave_layout_size
uint32_t spatial_wave_model_lds_probe()
{
    return (uint32_t)sp_wave_model_layout(FVB_MAX_PARAMS).n_doubles;
}
size_t spatial_wave_layout_size()
{
    return sizeof(WaveLayout);
}
} // namespace fvb
