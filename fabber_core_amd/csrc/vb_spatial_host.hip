// Spatial VB kernels for models that are evaluated on the host (HostLinModel, vb_models.h)
#include "vb_spatial.h"

#include <cstdlib>

namespace fvb
{
SpatialKernels get_spatial_kernels_host(int P, bool need_f)
{
    // more than 8 parameters: the wave-per-voxel family (vb_spatial_wave.h), up to FVB_MAX_PARAMS. FVB_SPATIAL_WIDE
    // (tests) takes it for every parameter count, so that it can be compared with the lane form on one problem.
    if (P > 8 || getenv("FVB_SPATIAL_WIDE"))
        return get_spatial_kernels_wide(P, need_f);
    switch (P)
    {
        FVB_SPATIAL_CASE(HostLinModel, "host", 1)
        FVB_SPATIAL_CASE(HostLinModel, "host", 2)
        FVB_SPATIAL_CASE(HostLinModel, "host", 3)
        FVB_SPATIAL_CASE(HostLinModel, "host", 4)
        FVB_SPATIAL_CASE(HostLinModel, "host", 5)
        FVB_SPATIAL_CASE(HostLinModel, "host", 6)
        FVB_SPATIAL_CASE(HostLinModel, "host", 7)
        FVB_SPATIAL_CASE(HostLinModel, "host", 8)
    default:
        return SpatialKernels{};
    }
}
} // namespace fvb
