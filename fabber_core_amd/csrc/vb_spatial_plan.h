/*
 * vb_spatial_plan.h - the planning half of the spatial VB host layer: everything that is integer work on the
 * co-ordinate list and the priors and needs no device. Neighbour table (Vb::CalcNeighbours, inference_vb.cc:830-964),
 * prior scan, sweep levels and their order, the slab-major numbering of the split sweep, the a_K segments, the prep
 * kernel's tiles and the z-slabs of a run on several devices. Plain C++17: no HIP include, no getenv - the switches
 * arrive as arguments (vb_spatial_run.h reads them). tests/cpp/test_spatial_plan.cc checks it on the CPU.
 */
#pragma once

#include "../../include/fabber_vb.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <string>
#include <thread>
#include <vector>

namespace fvb
{
namespace plan
{
// a value a test switch may force (set = false: the rule decides)
struct Forced
{
    bool set = false;
    int value = 0;
};

inline int sign_of(int x)
{
    return (x > 0) - (x < 0);
}

// First-neighbour table in the reference's order (+x, -x, +y, -y, +z, -z, limited by
// spatial-dims), -1 where there is no neighbour. Returns "" or an error message.
// dirs (optional): [V] which of the reference's six offsets (+x -x +y -y +z -z = 0 .. 5, inference_vb.cc:863-869) each
// listed neighbour was found with, 3 bits per list slot (7 = none): the split sweep's records are laid out by
// direction, and a sum over the listed neighbours in list order is then a sum over the directions in order
inline std::string build_neighbours(const int32_t *coords, int V, int dims, std::vector<int32_t> &nn, std::vector<int32_t> *dirs = nullptr)
{
    nn.assign((size_t)V * 6, -1);
    if (dirs)
        dirs->assign((size_t)V, 0777777);
    if (V == 0)
        return "";
    const int32_t *X = coords, *Y = coords + V, *Z = coords + 2 * (size_t)V;
    for (int v = 0; v + 1 < V; v++) // CheckCoordMatrixCorrectlyOrdered, :769-793
        if (sign_of(X[v + 1] - X[v]) + 10 * sign_of(Y[v + 1] - Y[v]) + 100 * sign_of(Z[v + 1] - Z[v]) <= 0)
            return "Coordinate matrix must be in correct order to use adjacency-based priors.";
    int xsize = 0, ysize = 0;
    for (int v = 0; v < V; v++)
    {
        xsize = std::max(xsize, (int)X[v] + 1);
        ysize = std::max(ysize, (int)Y[v] + 1);
    }
    std::vector<long long> offsets(V);
    for (int v = 0; v < V; v++)
        offsets[v] = (long long)Z[v] * xsize * ysize + (long long)Y[v] * xsize + X[v];
    const long long delta[6] = { 1, -1, xsize, -xsize, (long long)xsize * ysize, -(long long)xsize * ysize };
    const int max_delta = dims * 2 - 1;
    // The reference finds "the voxel at offset pos + delta" by binary search in the (sorted)
    // offsets. For a mask that fills a fair share of its bounding box the same question is one
    // look-up in a dense offset -> voxel map; the search is kept for sparse / odd geometries.
    const long long span = offsets[V - 1] - offsets[0] + 1;
    std::vector<int32_t> dense;
    if (span > 0 && span <= std::max<long long>(64LL * V, 1 << 20))
    {
        dense.assign((size_t)span, -1);
        for (int v = 0; v < V; v++)
            dense[(size_t)(offsets[v] - offsets[0])] = v;
    }
    auto find = [&](long long target) -> int {
        if (!dense.empty())
        {
            const long long rel = target - offsets[0];
            return (rel < 0 || rel >= span) ? -1 : dense[(size_t)rel];
        }
        auto it = std::lower_bound(offsets.begin(), offsets.end(), target);
        return (it == offsets.end() || *it != target) ? -1 : (int)(it - offsets.begin());
    };
    bool non_negative = true;
    for (int v = 0; v < V && non_negative; v++)
        non_negative = X[v] >= 0 && Y[v] >= 0 && Z[v] >= 0;
    if (non_negative && !dense.empty())
    {
        // With non-negative co-ordinates pos % xsize == x and pos % (xsize ysize) == y xsize + x,
        // so the four wrap-around tests (:906-925) read "x is on the last/first column" and "y is
        // on the last/first row"; and every relation found this way is mutual by construction
        // (the voxel found at pos + delta finds this one at its pos - delta), which is what the
        // reference verifies at :958-962.
        const long long base = offsets[0];
        for (int v = 0; v < V; v++)
        {
            const bool ok[6] = { X[v] < xsize - 1, X[v] > 0, Y[v] < ysize - 1, Y[v] > 0, true, true };
            const long long rel0 = offsets[v] - base;
            int32_t *row = &nn[(size_t)v * 6];
            int slot = 0;
            for (int n = 0; n <= max_delta; n++)
            {
                const long long rel = rel0 + delta[n];
                if (!ok[n] || rel < 0 || rel >= span)
                    continue;
                const int32_t found = dense[(size_t)rel];
                if (found >= 0)
                {
                    if (dirs)
                        (*dirs)[(size_t)v] = ((*dirs)[(size_t)v] & ~(7 << (3 * slot))) | (n << (3 * slot));
                    row[slot++] = found;
                }
            }
        }
        return "";
    }
    for (int v = 0; v < V; v++)
    {
        const long long pos = offsets[v];
        for (int n = 0; n <= max_delta; n++)
        {
            const int found = find(pos + delta[n]);
            if (found < 0)
                continue;
            if (n < 4) // wrap-around test, :906-925
            {
                bool ignore = false;
                if (delta[n] > 0)
                {
                    const long long test = delta[n + 2];
                    if (test > 0)
                        ignore = (pos % test) >= test - delta[n];
                }
                else
                {
                    const long long test = -delta[n + 2];
                    if (test > 0)
                        ignore = (pos % test) < -delta[n];
                }
                if (ignore)
                    continue;
            }
            // keep the reference's list order: entries are appended, so compact to the front
            int32_t *row = &nn[(size_t)v * 6];
            int slot = 0;
            while (row[slot] >= 0)
                slot++;
            row[slot] = (int32_t)found;
            if (dirs)
                (*dirs)[(size_t)v] = ((*dirs)[(size_t)v] & ~(7 << (3 * slot))) | (n << (3 * slot));
        }
    }
    // every neighbour relation must be mutual (:958-962)
    for (int v = 0; v < V; v++)
        for (int a = 0; a < 6 && nn[(size_t)v * 6 + a] >= 0; a++)
        {
            const int u = nn[(size_t)v * 6 + a];
            int back = 0;
            for (int b = 0; b < 6; b++)
                back += (nn[(size_t)u * 6 + b] == v);
            if (back != 1)
                return "Each of this voxel's neighbours must have this voxel as a neighbour";
        }
    return "";
}

// ---- the priors: what the sweeps have to order ----
struct PriorScan
{
    bool has_spatial = false;       // a prior of types M, m, P, p
    bool second_neighbours = false; // types P, p: the per-level kernel sums the neighbours of neighbours
    bool minus_zero = false;        // prec0 mean0 = -0 with a type P, p prior: the sign of the reference's 0 x sum
                                    // would decide the sign of a zero prior mean
    int n_spatial = 0;              // types M, m: the parameters the ordered part of the split sweep updates
    int spatial_param[FVB_MAX_PARAMS] = { 0 };
};
inline PriorScan scan_priors(int P, const int32_t *prior_type, const double *prior_prec, const double *prior_mean)
{
    PriorScan s;
    for (int k = 0; k < P; k++)
    {
        const bool second = (prior_type[k] == FVB_PRIOR_SPATIAL_P || prior_type[k] == FVB_PRIOR_SPATIAL_p);
        s.second_neighbours |= second;
        s.has_spatial |= prior_type[k] >= FVB_PRIOR_SPATIAL_M;
        const double pm0 = prior_prec[k] * prior_mean[k];
        s.minus_zero |= second && pm0 == 0 && std::signbit(pm0);
        if (prior_type[k] == FVB_PRIOR_SPATIAL_M || prior_type[k] == FVB_PRIOR_SPATIAL_m)
            s.spatial_param[s.n_spatial++] = k;
    }
    return s;
}

// A few host threads over contiguous ranges of n items (the passes are memory-bound scans of the co-ordinates);
// thread t takes [chunk(t), chunk(t + 1)), so thread order is index order.
struct HostThreads
{
    int n = 0, nt = 1;
    HostThreads(int n_items, Forced forced)
        : n(n_items)
    {
        nt = (n >= (1 << 18)) ? (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency())) : 1;
        if (forced.set) // tests: threads on small volumes
            nt = std::max(1, std::min(64, forced.value));
        nt = std::max(1, std::min(nt, std::max(n, 1)));
    }
    int chunk(int t) const
    {
        return (int)((long long)n * t / nt);
    }
    void parallel(const std::function<void(int)> &body) const
    {
        if (nt == 1)
            return body(0);
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; t++)
            pool.emplace_back(body, t);
        body(0);
        for (auto &th : pool)
            th.join();
    }
};

// the owned voxels [begin, end) of a local co-ordinate list [3][V]; item i of a pass is voxel begin + i
struct Owned
{
    const int32_t *X, *Y, *Z;
    int V, begin, end;
    Owned(const int32_t *coords, int V_, int begin_, int end_)
        : X(coords), Y(coords + V_), Z(coords + 2 * (size_t)V_), V(V_), begin(begin_), end(end_)
    {
    }
    int n() const
    {
        return end - begin;
    }
    bool whole() const
    {
        return begin == 0 && end == V;
    }
};

// Level function a x + b y + c z: a stencil offset that leads to a smaller voxel index must
// lower the level, one that leads to a larger index must raise it. First neighbours only: (1,1,1). Second
// neighbours too (the per-level kernel sums the neighbours of neighbours for types P, p, e.g. (x+1, y-1) which
// has a smaller index - the sum is multiplied by the 0 of priors.cc:455, but a NaN in it is not lost): b > a and
// c > b, so (1,2,3). The split form treats types P, p as local (vb_spatial.h) and numbers with (1,1,1).
struct Levels
{
    long long cy = 1, cz = 1, lmin = 0, lmax = 0;
    long long of(const Owned &o, int i) const
    {
        const int v = o.begin + i;
        return (long long)o.X[v] + cy * o.Y[v] + cz * o.Z[v];
    }
    long long range() const
    {
        return lmax - lmin;
    }
};
constexpr long long MAX_LEVEL_RANGE = 1LL << 22; // what a table indexed by level may span

inline Levels scan_levels(const Owned &o, long long cy, long long cz, const HostThreads &th)
{
    Levels lv;
    lv.cy = cy;
    lv.cz = cz;
    std::vector<long long> tmin(th.nt, 0), tmax(th.nt, 0);
    th.parallel([&](int t) {
        long long lo = 0, hi = 0;
        for (int i = th.chunk(t); i < th.chunk(t + 1); i++)
        {
            const long long l = lv.of(o, i);
            lo = (i == th.chunk(t) || l < lo) ? l : lo;
            hi = (i == th.chunk(t) || l > hi) ? l : hi;
        }
        tmin[t] = lo;
        tmax[t] = hi;
    });
    bool first = true;
    for (int t = 0; t < th.nt; t++)
        if (th.chunk(t + 1) > th.chunk(t))
        {
            lv.lmin = (first || tmin[t] < lv.lmin) ? tmin[t] : lv.lmin;
            lv.lmax = (first || tmax[t] > lv.lmax) ? tmax[t] : lv.lmax;
            first = false;
        }
    return lv;
}

// The level order (voxel ids sorted by level, index order within a level) is what the per-level launches walk:
// level l is order[level_begin[l] .. level_begin[l + 1]) and has the value level_value[l].
struct LevelOrder
{
    std::vector<int32_t> level_begin, order;
    std::vector<long long> level_value;
    int level_w[3] = { 1, 1, 1 };
};
// counting_limit: level ranges below it take the counting sort, the others std::stable_sort (same result)
inline LevelOrder build_level_order(const Owned &o, const Levels &lv, const HostThreads &th, long long counting_limit = MAX_LEVEL_RANGE)
{
    LevelOrder r;
    const int n_owned = o.n();
    r.order.assign(std::max(n_owned, 1), 0);
    r.level_w[1] = (int)lv.cy;
    r.level_w[2] = (int)lv.cz;
    if (lv.range() < counting_limit)
    {
        // counting sort (stable: voxels of a level stay in index order; per-thread histograms keep it so)
        const size_t nl = (size_t)(lv.range() + 1);
        std::vector<std::vector<int32_t> > count(th.nt, std::vector<int32_t>(nl, 0));
        th.parallel([&](int t) {
            int32_t *c = count[t].data();
            for (int i = th.chunk(t); i < th.chunk(t + 1); i++)
                c[(size_t)(lv.of(o, i) - lv.lmin)]++;
        });
        int32_t running = 0;
        for (size_t l = 0; l < nl; l++)
        {
            const int32_t begin = running;
            for (int t = 0; t < th.nt; t++) // thread order = index order
            {
                const int32_t n = count[t][l];
                count[t][l] = running; // becomes this thread's first slot in level l
                running += n;
            }
            if (running > begin)
            {
                r.level_begin.push_back(begin);
                r.level_value.push_back(lv.lmin + (long long)l);
            }
        }
        r.level_begin.push_back(n_owned);
        th.parallel([&](int t) {
            int32_t *c = count[t].data();
            for (int i = th.chunk(t); i < th.chunk(t + 1); i++)
                r.order[c[(size_t)(lv.of(o, i) - lv.lmin)]++] = o.begin + i;
        });
    }
    else
    {
        std::vector<int32_t> idx(n_owned);
        for (int i = 0; i < n_owned; i++)
            idx[i] = i;
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return lv.of(o, a) < lv.of(o, b); });
        for (int i = 0; i < n_owned; i++)
        {
            if (i == 0 || lv.of(o, idx[i]) != lv.of(o, idx[i - 1]))
            {
                r.level_begin.push_back(i);
                r.level_value.push_back(lv.of(o, idx[i]));
            }
            r.order[i] = o.begin + idx[i];
        }
        r.level_begin.push_back(n_owned);
    }
    return r;
}

// ---- slab-major numbering of the split first sweep (vb_spatial.h, "slab form") ----
// A slab = dz z-planes, inside a slab the voxels level by level (index order in a level); key = (slab, level) of a
// voxel, a run = the voxels of a key. dz: as few planes as keep the slabs within the chip's workgroups (every slab is
// one resident workgroup): one plane per slab up to 192 planes. Thicker slabs mean fewer hand-overs between workgroups
// (2.4 us each, one after the other) but longer runs and fewer groups per workgroup to hide the records'
// latency: measured at 128^3, 0.51 ms per sweep with dz = 1, 0.65 with 2, 0.94 with 3, 1.04 with 4.
constexpr int32_t NP_BELOW = -2, NP_ABOVE = -3; // a ghost's entry in pos_of (= FVB_NP_BELOW / FVB_NP_ABOVE of vb_spatial.h)
constexpr int MAX_SLAB_RUN = 8192;

// The sweep's workgroups (1024 lanes, up to 128 KB of LDS: one per compute unit) wait for the slab below.
// Workgroups are dispatched in index order, so the one waited for is resident or finished; all the same the
// count stays within what THIS device (a partition of the chip in CPX mode has 32 compute units, not 256)
// holds at once, three quarters of it at most, shared between the runs that sweep on it together. A wait
// that does not end gives up (slab_wait_inbox) and the run is repeated with the per-level launches.
inline long long slab_cap(int compute_units, int device_share)
{
    return std::max(1LL, std::min(192LL, (long long)compute_units * 3 / 4 / std::max(1, device_share)));
}

struct SlabParams
{
    int zmin = 0;
    long long lmin = 0, dz = 1, n_slabs = 0;
    size_t nl = 0; // levels a slab may hold: keys = n_slabs * nl
    size_t n_keys() const
    {
        return (size_t)n_slabs * nl;
    }
    size_t key(int x, int y, int z) const // (levels of the split sweep: x + y + z)
    {
        return (size_t)((z - zmin) / dz) * nl + (size_t)((long long)x + y + z - lmin);
    }
    // whether a table over the keys is reasonable at all
    bool usable(int spatial_dims) const
    {
        return spatial_dims <= 3 && n_slabs * (long long)nl <= (1LL << 21);
    }
};
inline SlabParams slab_params(int zmin, int zmax, const Levels &lv, long long cap, Forced forced_dz)
{
    SlabParams p;
    const long long nz = (long long)zmax - zmin + 1;
    p.zmin = zmin;
    p.lmin = lv.lmin;
    p.dz = std::max(1LL, (nz + cap - 1) / cap);
    if (forced_dz.set)
        p.dz = std::max((nz + cap - 1) / cap, (long long)std::max(1, forced_dz.value));
    p.n_slabs = (nz + p.dz - 1) / p.dz;
    p.nl = (size_t)(lv.range() + 1);
    return p;
}

struct SlabNumbering
{
    std::vector<int32_t> pos_of;                             // [V] position of every owned voxel (host numbering)
    std::vector<int32_t> level_pos, level_count, slab_first; // first position and length of every run; first run of every slab
    int sl_max_run = 0;
};

// voxels per key, one histogram per thread
inline std::vector<std::vector<int32_t> > slab_count(const Owned &o, const SlabParams &p, const HostThreads &th)
{
    std::vector<std::vector<int32_t> > count(th.nt, std::vector<int32_t>(p.n_keys(), 0));
    th.parallel([&](int t) {
        int32_t *c = count[t].data();
        for (int i = th.chunk(t); i < th.chunk(t + 1); i++)
            c[p.key(o.X[o.begin + i], o.Y[o.begin + i], o.Z[o.begin + i])]++;
    });
    return count;
}
// The prefix pass: count[t][key] becomes the first position of thread t's voxels of that key (thread order = index
// order); the runs that are not empty, slab by slab.
inline SlabNumbering slab_prefix(std::vector<std::vector<int32_t> > &count, const SlabParams &p)
{
    SlabNumbering s;
    s.slab_first.assign((size_t)p.n_slabs + 1, 0);
    int32_t running = 0;
    for (size_t key = 0; key < p.n_keys(); key++)
    {
        if (key % p.nl == 0)
            s.slab_first[key / p.nl] = (int32_t)s.level_pos.size();
        const int32_t begin = running;
        for (auto &c : count)
        {
            const int32_t n = c[key];
            c[key] = running;
            running += n;
        }
        if (running > begin)
        {
            s.level_pos.push_back(begin);
            s.level_count.push_back(running - begin);
            s.sl_max_run = std::max(s.sl_max_run, (int)(running - begin));
        }
    }
    s.slab_first[(size_t)p.n_slabs] = (int32_t)s.level_pos.size();
    return s;
}
// whether the sweep kernel takes the numbering: a run fits its LDS, every slab is a resident workgroup
inline bool slab_accepted(const SlabNumbering &s, const SlabParams &p, long long cap)
{
    return s.sl_max_run <= MAX_SLAB_RUN && p.n_slabs <= cap;
}
// the positions of the owned voxels, from the first positions slab_prefix left in count
inline void slab_place(const Owned &o, const SlabParams &p, const HostThreads &th, std::vector<std::vector<int32_t> > &count,
    std::vector<int32_t> &pos_of)
{
    pos_of.assign((size_t)o.V, 0);
    th.parallel([&](int t) {
        int32_t *c = count[t].data();
        for (int i = th.chunk(t); i < th.chunk(t + 1); i++)
            pos_of[(size_t)o.begin + i] = c[p.key(o.X[o.begin + i], o.Y[o.begin + i], o.Z[o.begin + i])]++;
    });
}
// ghosts have no position: what stands in sw_npos for them says where their mean comes from (vb_spatial.h)
inline void mark_ghosts(const Owned &o, std::vector<int32_t> &pos_of)
{
    for (int v = 0; v < o.begin; v++)
        pos_of[(size_t)v] = NP_BELOW;
    for (int v = o.end; v < o.V; v++)
        pos_of[(size_t)v] = NP_ABOVE;
}
// lanes per run: the next power of two from 64 that holds the longest run, 1024 at most
inline int slab_width(int sl_max_run, Forced forced)
{
    int w = 64;
    while (w < sl_max_run && w < 1024)
        w *= 2;
    if (forced.set) // tests: lanes that take several voxels of a run
        w = std::max(64, std::min(1024, forced.value / 64 * 64));
    if (1024 % w != 0) // (the 1024 lanes are whole groups)
        w = 64;
    return w;
}
inline int max_runs_per_slab(const std::vector<int32_t> &slab_first)
{
    int m = 0;
    for (size_t b = 0; b + 1 < slab_first.size(); b++)
        m = std::max(m, (int)(slab_first[b + 1] - slab_first[b]));
    return m;
}
// The whole numbering on the host (levels: scan_levels with (1,1,1)). Returns false - and an empty numbering - where
// the sweep kernel does not take it.
inline bool number_slabs(const Owned &o, const Levels &lv, long long cap, Forced forced_dz, int spatial_dims, const HostThreads &th,
    SlabParams &p, SlabNumbering &s)
{
    int zmin = o.Z[o.begin], zmax = o.Z[o.begin];
    for (int v = o.begin; v < o.end; v++)
    {
        zmin = std::min(zmin, (int)o.Z[v]);
        zmax = std::max(zmax, (int)o.Z[v]);
    }
    p = slab_params(zmin, zmax, lv, cap, forced_dz);
    s = SlabNumbering();
    if (!p.usable(spatial_dims))
        return false;
    std::vector<std::vector<int32_t> > count = slab_count(o, p, th);
    s = slab_prefix(count, p);
    if (!slab_accepted(s, p, cap))
    {
        s = SlabNumbering();
        return false;
    }
    slab_place(o, p, th, count, s.pos_of);
    return true;
}

// segments of the a_K sums: every z-plane of the owned voxels, cut every 4096 voxels from its first
inline std::vector<int32_t> ak_segments(const Owned &o)
{
    std::vector<int32_t> seg_start;
    for (int v = o.begin; v < o.end; v++)
        if (v == o.begin || o.Z[v] != o.Z[v - 1] || v - seg_start.back() >= 4096)
            seg_start.push_back(v);
    seg_start.push_back(o.end);
    return seg_start;
}

// the prep kernel's 8 x 8 tiles of the planes z0 .. z1 of a box xsize x ysize (vb_spatial.h); n_tiles = 0: a mask
// that fills little of its box would spend the kernel on empty tiles
struct PrepTiles
{
    int32_t tile_nx = 0, tile_ny = 0, tile_z0 = 0, n_tiles = 0;
};
inline PrepTiles prep_tiles(int xsize, int ysize, long long z0, long long z1, int n_owned)
{
    PrepTiles t;
    const long long tnx = (xsize + 7) / 8, tny = (ysize + 7) / 8, tiles = (z1 - z0 + 1) * tnx * tny;
    if (tiles > 0 && tiles * 64 <= 4LL * n_owned + 4096 && tiles < (1LL << 30))
    {
        t.tile_nx = (int32_t)tnx;
        t.tile_ny = (int32_t)tny;
        t.tile_z0 = (int32_t)z0;
        t.n_tiles = (int32_t)tiles;
    }
    return t;
}

// ---- the z-slabs of a run on several devices: cuts on z-plane boundaries, balanced by voxel count ----
struct SlabCut
{
    int g0, b, e, g1; // local list = global voxels [g0, g1), owned [b, e)
};
// first voxel of every z-plane; false where z decreases along the list
inline bool plane_starts(const int32_t *Z, int V, std::vector<int> &plane_start)
{
    plane_start.clear();
    for (int v = 0; v < V; v++)
    {
        if (v > 0 && Z[v] < Z[v - 1])
            return false;
        if (v == 0 || Z[v] != Z[v - 1])
            plane_start.push_back(v);
    }
    return true;
}
// Every slab keeps at least `halo` planes (its neighbours' ghosts must not reach past it) and leaves as many for
// each slab after it; within that the cut falls on the plane boundary nearest to an equal share of the voxels.
// A decomposition that does not work out (a very unbalanced mask, planes missing from the z range) is tried
// again with one slab fewer, down to the one-device run - never refused.
inline std::vector<SlabCut> slab_cuts(const int32_t *Z, int V, const std::vector<int> &plane_start, int max_slabs, int halo)
{
    const int n_planes = (int)plane_start.size();
    int world = (int)std::min<size_t>((size_t)max_slabs, std::max<size_t>(1, plane_start.size() / (size_t)(2 * halo)));
    for (; world > 1; world--)
    {
        std::vector<int> cut(1, 0); // plane index at which slab r starts
        for (int r = 1; r < world; r++)
        {
            const int lo = cut.back() + halo, hi = n_planes - (world - r) * halo;
            const double want = (double)V * r / world;
            int best = lo;
            for (int p = lo; p <= hi; p++)
                if (std::fabs(plane_start[p] - want) < std::fabs(plane_start[best] - want))
                    best = p;
            cut.push_back(best);
        }
        std::vector<int> bounds;
        for (int c : cut)
            bounds.push_back(plane_start[c]);
        bounds.push_back(V);
        std::vector<SlabCut> slabs;
        bool fits = true;
        for (int r = 0; r < world && fits; r++)
        {
            SlabCut sl = { bounds[r], bounds[r], bounds[r + 1], bounds[r + 1] };
            if (r > 0)
                sl.g0 = (int)(std::lower_bound(Z, Z + V, Z[sl.b] - halo) - Z);
            if (r < world - 1)
                sl.g1 = (int)(std::upper_bound(Z, Z + V, Z[sl.e - 1] + halo) - Z);
            fits = !((r > 0 && sl.g0 < bounds[r - 1]) || (r < world - 1 && sl.g1 > bounds[r + 2]));
            slabs.push_back(sl);
        }
        if (fits)
            return slabs;
    }
    return std::vector<SlabCut>(1, SlabCut{ 0, 0, V, V });
}
// the most voxels a slab exchanges with a neighbour
inline int max_halo(const std::vector<SlabCut> &slabs)
{
    int m = 1;
    for (const SlabCut &sl : slabs)
        m = std::max(m, std::max(sl.b - sl.g0, sl.g1 - sl.e));
    return m;
}
} // namespace plan
} // namespace fvb
