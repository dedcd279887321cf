/*
 * vb_spatial_geom.h - the geometry of a spatial VB run worked out on the device: the first-neighbour table
 * (plan::build_neighbours of vb_spatial_plan.h for the usual geometry) and the two kernels of the slab-major
 * numbering. Included by vb_spatial_api.hip only.
 */
#pragma once

#include "vb_spatial_run.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <string>

namespace
{
// For the usual geometry (non-negative co-ordinates, a mask that fills a fair share of its bounding
// box) the table is a handful of independent look-ups per voxel: 22 ms of single-threaded host
// time plus a 50 MB upload for 128^3 voxels, well under a millisecond as three kernels on the
// co-ordinates (24 MB upload). Anything else takes the host path (plan::build_neighbours).
struct GeomScan
{
    int32_t xmax, ymax, cmin, bad_order;
    int32_t zmin, zmax, lmin, lmax; // z and x + y + z: what the slab numbering of the split sweep needs
};

__global__ __launch_bounds__(256) void geom_scan_kernel(const int32_t *coords, int V, GeomScan *out)
{
    const int32_t *X = coords, *Y = coords + V, *Z = coords + 2 * (size_t)V;
    int xmax = 0, ymax = 0, cmin = 0, bad = 0;
    int zmin = INT_MAX, zmax = INT_MIN, lmin = INT_MAX, lmax = INT_MIN;
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x)
    {
        xmax = max(xmax, X[v]);
        ymax = max(ymax, Y[v]);
        cmin = min(cmin, min(X[v], min(Y[v], Z[v])));
        zmin = min(zmin, Z[v]);
        zmax = max(zmax, Z[v]);
        lmin = min(lmin, X[v] + Y[v] + Z[v]);
        lmax = max(lmax, X[v] + Y[v] + Z[v]);
        if (v + 1 < V) // CheckCoordMatrixCorrectlyOrdered, inference_vb.cc:769-793
        {
            const int dx = X[v + 1] - X[v], dy = Y[v + 1] - Y[v], dz = Z[v + 1] - Z[v];
            const int key = ((dx > 0) - (dx < 0)) + 10 * ((dy > 0) - (dy < 0)) + 100 * ((dz > 0) - (dz < 0));
            bad |= (key <= 0);
        }
    }
    atomicMax(&out->xmax, xmax);
    atomicMax(&out->ymax, ymax);
    atomicMin(&out->cmin, cmin);
    atomicMin(&out->zmin, zmin);
    atomicMax(&out->zmax, zmax);
    atomicMin(&out->lmin, lmin);
    atomicMax(&out->lmax, lmax);
    if (bad)
        atomicOr(&out->bad_order, 1);
}

// Slab-major numbering of the split sweep on the device (vb_spatial.h, "slab form"): key = (slab, level) of a voxel;
// a histogram, the prefix sums (on the host: a few ten thousand keys) and one more pass that hands out the positions
// of a key's run in arrival order - which voxel of a run gets which of its positions changes no result.
__device__ __forceinline__ int slab_key(const int32_t *coords, int V, int v, int zmin, int dz, int lmin, int nl)
{
    const int x = coords[v], y = coords[(size_t)V + v], z = coords[2 * (size_t)V + v];
    return ((z - zmin) / dz) * nl + (x + y + z - lmin);
}
__global__ __launch_bounds__(256) void slab_count_kernel(const int32_t *coords, int V, int zmin, int dz, int lmin, int nl, int32_t *count)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < V)
        atomicAdd(count + slab_key(coords, V, v, zmin, dz, lmin, nl), 1);
}
__global__ __launch_bounds__(256) void slab_place_kernel(const int32_t *coords, int V, int zmin, int dz, int lmin, int nl, int32_t *next,
    int32_t *pos_of)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < V)
        pos_of[v] = atomicAdd(next + slab_key(coords, V, v, zmin, dz, lmin, nl), 1);
}

__global__ __launch_bounds__(256) void geom_dense_kernel(const int32_t *coords, int V, int xsize, int ysize, long long base,
    int32_t *dense)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V)
        return;
    const long long off = (long long)coords[2 * (size_t)V + v] * xsize * ysize + (long long)coords[(size_t)V + v] * xsize + coords[v];
    dense[off - base] = v;
}

// Vb::CalcNeighbours (inference_vb.cc:830-964) for non-negative co-ordinates: the wrap-around tests
// (:906-925) read "x is on the last / first column", "y is on the last / first row"
__global__ __launch_bounds__(256) void geom_neighbours_kernel(const int32_t *coords, int V, int xsize, int ysize, long long base,
    long long span, int max_delta, const int32_t *dense, int32_t *nn, int32_t *dirs)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V)
        return;
    const int x = coords[v], y = coords[(size_t)V + v], z = coords[2 * (size_t)V + v];
    const long long rel0 = (long long)z * xsize * ysize + (long long)y * xsize + x - base;
    const long long delta[6] = { 1, -1, xsize, -xsize, (long long)xsize * ysize, -(long long)xsize * ysize };
    const bool ok[6] = { x < xsize - 1, x > 0, y < ysize - 1, y > 0, true, true };
    int32_t row[6] = { -1, -1, -1, -1, -1, -1 };
    int slot = 0;
    int32_t dir = 0777777; // (see build_neighbours)
#pragma unroll
    for (int n = 0; n < 6; n++)
    {
        const long long rel = rel0 + delta[n];
        if (n > max_delta || !ok[n] || rel < 0 || rel >= span)
            continue;
        const int32_t found = dense[rel];
        if (found >= 0)
        {
#pragma unroll
            for (int q = 0; q < 6; q++) // (compile-time indices: the row stays in registers)
                if (q == slot)
                    row[q] = found;
            dir = (dir & ~(7 << (3 * slot))) | (n << (3 * slot));
            slot++;
        }
    }
    dirs[v] = dir;
#pragma unroll
    for (int q = 0; q < 6; q++)
        nn[(size_t)v * 6 + q] = row[q];
}

// Returns 0 (d_nn filled), 1 (geometry not suited: use the host path) or a negative error code.
int build_neighbours_device(const int32_t *h_coords, int V, int dims, int32_t *d_nn, int32_t *d_dirs, hipStream_t stream, std::string &err,
    fvb::DevMem *keep_coords = nullptr, GeomScan *scan_out = nullptr, fvb::DenseMap *keep_dense = nullptr)
{
#define FVB_GEOM_CHECK(expr)                                                                                 \
    do                                                                                                       \
    {                                                                                                        \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
        {                                                                                                    \
            err = std::string(#expr) + ": " + hipGetErrorString(e_);                                         \
            return -100 - (int)e_;                                                                           \
        }                                                                                                    \
    } while (0)
    fvb::DevMem d_coords, d_scan, d_dense;
    FVB_GEOM_CHECK(d_coords.alloc(sizeof(int32_t) * 3 * (size_t)V, stream));
    FVB_GEOM_CHECK(d_scan.alloc(sizeof(GeomScan), stream));
    FVB_GEOM_CHECK(hipMemcpyAsync(d_coords.p, h_coords, sizeof(int32_t) * 3 * (size_t)V, hipMemcpyHostToDevice, stream));
    GeomScan scan0 = { 0, 0, 0, 0, INT_MAX, INT_MIN, INT_MAX, INT_MIN };
    FVB_GEOM_CHECK(hipMemcpyAsync(d_scan.p, &scan0, sizeof(GeomScan), hipMemcpyHostToDevice, stream));
    FVB_GEOM_CHECK(hipStreamSynchronize(stream)); // (scan0 is a local)
    const unsigned blocks = (unsigned)std::min(1024, (V + 255) / 256);
    hipLaunchKernelGGL(geom_scan_kernel, dim3(blocks), dim3(256), 0, stream, (const int32_t *)d_coords.p, V, (GeomScan *)d_scan.p);
    GeomScan scan;
    FVB_GEOM_CHECK(hipMemcpyAsync(&scan, d_scan.p, sizeof(scan), hipMemcpyDeviceToHost, stream));
    FVB_GEOM_CHECK(hipStreamSynchronize(stream));
    if (scan.bad_order)
    {
        err = "Coordinate matrix must be in correct order to use adjacency-based priors.";
        return -41;
    }
    if (scan.cmin < 0)
        return 1;
    const int xsize = scan.xmax + 1, ysize = scan.ymax + 1;
    const int32_t *X = h_coords, *Y = h_coords + V, *Z = h_coords + 2 * (size_t)V;
    const long long first = (long long)Z[0] * xsize * ysize + (long long)Y[0] * xsize + X[0];
    const long long last = (long long)Z[V - 1] * xsize * ysize + (long long)Y[V - 1] * xsize + X[V - 1];
    const long long span = last - first + 1;
    if (span <= 0 || span > std::max<long long>(64LL * V, 1 << 20))
        return 1;
    FVB_GEOM_CHECK(d_dense.alloc(sizeof(int32_t) * (size_t)span, stream));
    FVB_GEOM_CHECK(hipMemsetAsync(d_dense.p, 0xff, sizeof(int32_t) * (size_t)span, stream)); // -1
    const unsigned grid = (unsigned)((V + 255) / 256);
    hipLaunchKernelGGL(geom_dense_kernel, dim3(grid), dim3(256), 0, stream, (const int32_t *)d_coords.p, V, xsize, ysize, first,
        (int32_t *)d_dense.p);
    hipLaunchKernelGGL(geom_neighbours_kernel, dim3(grid), dim3(256), 0, stream, (const int32_t *)d_coords.p, V, xsize, ysize,
        first, span, dims * 2 - 1, (const int32_t *)d_dense.p, d_nn, d_dirs);
    FVB_GEOM_CHECK(hipGetLastError());
    FVB_GEOM_CHECK(hipStreamSynchronize(stream)); // the temporaries are freed on return
#undef FVB_GEOM_CHECK
    if (scan_out)
        *scan_out = scan;
    if (keep_coords) // the caller goes on with the co-ordinates on the device (slab numbering)
    {
        std::swap(keep_coords->p, d_coords.p);
        std::swap(keep_coords->stream, d_coords.stream);
    }
    if (keep_dense) // ... and with the map from box offsets to voxels (the prep kernel's tiles)
    {
        std::swap(keep_dense->map.p, d_dense.p);
        std::swap(keep_dense->map.stream, d_dense.stream);
        keep_dense->base = first;
        keep_dense->span = span;
        keep_dense->xsize = xsize;
        keep_dense->ysize = ysize;
    }
    return 0;
}
} // namespace
