// The planning half of the spatial VB host layer (fabber_core_amd/csrc/vb_spatial_plan.h) on the CPU: neighbour table,
// level order, slab-major numbering, a_K segments, prep tiles and the z-slabs of a run on several devices, each checked
// against a brute-force statement of what it has to be. Built with g++ alone: the header includes nothing of HIP.
#include "vb_spatial_plan.h"

#include <cstdio>
#include <map>
#include <numeric>
#include <random>
#include <set>
#include <tuple>

using namespace fvb::plan;

static int g_failures = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do                                                                                                       \
    {                                                                                                        \
        g_checks++;                                                                                          \
        if (!(cond))                                                                                         \
        {                                                                                                    \
            if (++g_failures <= 20)                                                                          \
                printf("FAILED %s:%d [%s]: %s\n", __FILE__, __LINE__, g_case.c_str(), #cond);                \
        }                                                                                                    \
    } while (0)
static std::string g_case;

// a voxel list [3][V] in the reference's order (x fastest, then y, then z)
struct Volume
{
    std::string name;
    std::vector<int32_t> coords;
    int V = 0;
    const int32_t *X() const { return coords.data(); }
    const int32_t *Y() const { return coords.data() + V; }
    const int32_t *Z() const { return coords.data() + 2 * (size_t)V; }
};
// keep: share of the box's voxels in the mask (seeded); skip_z: planes left out altogether
static Volume make_volume(const std::string &name, int nx, int ny, int nz, double keep, unsigned seed, const std::set<int> &skip_z = {})
{
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::vector<int32_t> x, y, z;
    for (int k = 0; k < nz; k++)
        for (int j = 0; j < ny; j++)
            for (int i = 0; i < nx; i++)
                if (!skip_z.count(k) && (keep >= 1.0 || u(rng) < keep))
                {
                    x.push_back(i);
                    y.push_back(j);
                    z.push_back(k);
                }
    Volume vol;
    vol.name = name;
    vol.V = (int)x.size();
    vol.coords = x;
    vol.coords.insert(vol.coords.end(), y.begin(), y.end());
    vol.coords.insert(vol.coords.end(), z.begin(), z.end());
    return vol;
}
static Forced forced(int value)
{
    Forced f;
    f.set = true;
    f.value = value;
    return f;
}

// ---- neighbour table: a search over the co-ordinates, direction by direction ----
static void check_neighbours(const Volume &vol)
{
    std::map<std::tuple<int, int, int>, int> at;
    for (int v = 0; v < vol.V; v++)
        at[std::make_tuple(vol.X()[v], vol.Y()[v], vol.Z()[v])] = v;
    const int d[6][3] = { { 1, 0, 0 }, { -1, 0, 0 }, { 0, 1, 0 }, { 0, -1, 0 }, { 0, 0, 1 }, { 0, 0, -1 } };
    for (int dims = 0; dims <= 3; dims++)
    {
        g_case = vol.name + " neighbours dims=" + std::to_string(dims);
        std::vector<int32_t> nn, dirs;
        CHECK(build_neighbours(vol.coords.data(), vol.V, dims, nn, &dirs).empty());
        CHECK(nn.size() == (size_t)vol.V * 6 && dirs.size() == (size_t)vol.V);
        bool same = nn.size() == (size_t)vol.V * 6, same_dirs = true;
        for (int v = 0; v < vol.V && same; v++)
        {
            int32_t want[6] = { -1, -1, -1, -1, -1, -1 }, want_dir = 0777777;
            int slot = 0;
            for (int n = 0; n < 2 * dims; n++)
            {
                auto it = at.find(std::make_tuple(vol.X()[v] + d[n][0], vol.Y()[v] + d[n][1], vol.Z()[v] + d[n][2]));
                if (it == at.end())
                    continue;
                want_dir = (want_dir & ~(7 << (3 * slot))) | (n << (3 * slot));
                want[slot++] = it->second;
            }
            for (int a = 0; a < 6; a++)
                same = same && nn[(size_t)v * 6 + a] == want[a];
            same_dirs = same_dirs && dirs[(size_t)v] == want_dir;
        }
        CHECK(same);
        CHECK(same_dirs);
        std::vector<int32_t> nn_only;
        CHECK(build_neighbours(vol.coords.data(), vol.V, dims, nn_only).empty() && nn_only == nn);
    }
    if (vol.V >= 4) // two voxels out of order
    {
        g_case = vol.name + " misordered";
        Volume bad = vol;
        for (int dim = 0; dim < 3; dim++)
            std::swap(bad.coords[(size_t)dim * vol.V + 1], bad.coords[(size_t)dim * vol.V + 2]);
        std::vector<int32_t> nn;
        CHECK(build_neighbours(bad.coords.data(), bad.V, 3, nn) == "Coordinate matrix must be in correct order to use adjacency-based priors.");
    }
}

static bool same_order(const LevelOrder &a, const LevelOrder &b)
{
    return a.level_begin == b.level_begin && a.level_value == b.level_value && a.order == b.order && a.level_w[0] == b.level_w[0]
        && a.level_w[1] == b.level_w[1] && a.level_w[2] == b.level_w[2];
}

// ---- level order of the owned range [begin, end) ----
static void check_level_order(const Volume &vol, int begin, int end)
{
    const Owned own(vol.coords.data(), vol.V, begin, end);
    std::vector<int32_t> nn;
    CHECK(build_neighbours(vol.coords.data(), vol.V, 3, nn).empty());
    for (int second = 0; second <= 1; second++)
    {
        g_case = vol.name + " level order [" + std::to_string(begin) + "," + std::to_string(end) + ") weights " + (second ? "(1,2,3)" : "(1,1,1)");
        const long long cy = second ? 2 : 1, cz = second ? 3 : 1;
        const HostThreads one(own.n(), forced(1));
        const Levels lv = scan_levels(own, cy, cz, one);
        const LevelOrder lo = build_level_order(own, lv, one);
        CHECK(lo.level_w[0] == 1 && lo.level_w[1] == cy && lo.level_w[2] == cz);
        // the same from every number of threads, and from both sorts
        for (int nt : { 1, 3, 7 })
        {
            const HostThreads th(own.n(), forced(nt));
            const Levels lt = scan_levels(own, cy, cz, th);
            CHECK(lt.lmin == lv.lmin && lt.lmax == lv.lmax);
            CHECK(same_order(lo, build_level_order(own, lt, th)));
            CHECK(same_order(lo, build_level_order(own, lt, th, 0))); // std::stable_sort
        }
        // a permutation of the owned range, level by level in rising order, index order within a level
        CHECK(lo.order.size() == (size_t)std::max(own.n(), 1));
        CHECK(lo.level_begin.size() == lo.level_value.size() + 1 && lo.level_begin.back() == own.n());
        std::vector<int> seen(vol.V, 0);
        std::vector<long long> level_of(vol.V, 0);
        bool sorted = true, right_level = true;
        for (size_t l = 0; l + 1 < lo.level_begin.size(); l++)
        {
            CHECK(lo.level_begin[l] < lo.level_begin[l + 1]);
            if (l > 0)
                CHECK(lo.level_value[l] > lo.level_value[l - 1]);
            for (int i = lo.level_begin[l]; i < lo.level_begin[l + 1]; i++)
            {
                const int v = lo.order[i];
                if (v < begin || v >= end)
                {
                    right_level = false;
                    continue;
                }
                seen[v]++;
                level_of[v] = lo.level_value[l];
                right_level = right_level && lo.level_value[l] == vol.X()[v] + cy * vol.Y()[v] + cz * vol.Z()[v];
                sorted = sorted && (i == lo.level_begin[l] || lo.order[i - 1] < v);
            }
        }
        bool permutation = true;
        for (int v = 0; v < vol.V; v++)
            permutation = permutation && seen[v] == ((v >= begin && v < end) ? 1 : 0);
        CHECK(permutation);
        CHECK(sorted);
        CHECK(right_level);
        if (own.n() > 0)
            CHECK(lo.level_value.front() == lv.lmin && lo.level_value.back() == lv.lmax);
        // what a voxel reads from voxels before it in the list has been swept at a lower level
        bool first_ok = true, second_ok = true;
        for (int v = begin; v < end; v++)
            for (int a = 0; a < 6; a++)
            {
                const int u = nn[(size_t)v * 6 + a];
                if (u < 0)
                    continue;
                if (u < v && u >= begin)
                    first_ok = first_ok && level_of[u] < level_of[v];
                for (int b = 0; b < 6 && second; b++)
                {
                    const int w = nn[(size_t)u * 6 + b];
                    if (w >= begin && w < v)
                        second_ok = second_ok && level_of[w] < level_of[v];
                }
            }
        CHECK(first_ok);
        CHECK(second_ok);
    }
}

// ---- slab-major numbering of the owned range ----
static void check_slab_numbering(const Volume &vol, int begin, int end)
{
    const Owned own(vol.coords.data(), vol.V, begin, end);
    if (own.n() == 0)
        return;
    for (int dz = 1; dz <= 3; dz++)
    {
        g_case = vol.name + " slab numbering [" + std::to_string(begin) + "," + std::to_string(end) + ") dz=" + std::to_string(dz);
        const long long cap = 192;
        SlabParams p;
        SlabNumbering s;
        const HostThreads one(own.n(), forced(1));
        const Levels lv = scan_levels(own, 1, 1, one);
        CHECK(number_slabs(own, lv, cap, forced(dz), 3, one, p, s));
        CHECK(p.dz == dz);
        for (int nt : { 3, 7 })
        {
            SlabParams pt;
            SlabNumbering st;
            const HostThreads th(own.n(), forced(nt));
            CHECK(number_slabs(own, scan_levels(own, 1, 1, th), cap, forced(dz), 3, th, pt, st));
            CHECK(st.pos_of == s.pos_of && st.level_pos == s.level_pos && st.level_count == s.level_count && st.slab_first == s.slab_first
                && st.sl_max_run == s.sl_max_run && pt.n_slabs == p.n_slabs && pt.nl == p.nl && pt.zmin == p.zmin);
        }
        // slab-major, level-major inside a slab, index order inside a run: the rank in that order is the position
        int zmin = vol.Z()[begin];
        for (int v = begin; v < end; v++)
            zmin = std::min(zmin, (int)vol.Z()[v]);
        auto slab_of = [&](int v) { return (vol.Z()[v] - zmin) / dz; };
        auto level_of = [&](int v) { return vol.X()[v] + vol.Y()[v] + vol.Z()[v]; };
        std::vector<int> by_key(own.n());
        std::iota(by_key.begin(), by_key.end(), begin);
        std::stable_sort(by_key.begin(), by_key.end(), [&](int a, int b) {
            return std::make_pair(slab_of(a), level_of(a)) < std::make_pair(slab_of(b), level_of(b));
        });
        CHECK(s.pos_of.size() == (size_t)vol.V);
        bool ranks = true;
        for (int i = 0; i < own.n(); i++)
            ranks = ranks && s.pos_of[by_key[i]] == i; // (a permutation of [0, n_owned) with it)
        CHECK(ranks);
        // the runs, the first run of every slab, the longest run
        std::vector<int32_t> run_pos, run_count, first_run;
        int longest = 0;
        for (int i = 0; i < own.n(); i++)
        {
            const bool new_run = i == 0 || slab_of(by_key[i]) != slab_of(by_key[i - 1]) || level_of(by_key[i]) != level_of(by_key[i - 1]);
            if (new_run)
            {
                run_pos.push_back(i);
                run_count.push_back(0);
            }
            while ((int)first_run.size() <= slab_of(by_key[i])) // (a slab without voxels starts where the next one does)
                first_run.push_back((int32_t)run_pos.size() - 1);
            longest = std::max(longest, ++run_count.back());
        }
        while ((long long)first_run.size() <= p.n_slabs)
            first_run.push_back((int32_t)run_pos.size());
        CHECK(s.level_pos == run_pos);
        CHECK(s.level_count == run_count);
        CHECK(s.slab_first == first_run);
        CHECK(s.sl_max_run == longest);
        CHECK(max_runs_per_slab(s.slab_first) <= (int)p.nl);
        // ghosts get the two markers, the owned voxels keep their positions
        std::vector<int32_t> marked = s.pos_of;
        mark_ghosts(own, marked);
        bool ghosts = true;
        for (int v = 0; v < vol.V; v++)
            ghosts = ghosts && marked[v] == (v < begin ? NP_BELOW : (v >= end ? NP_ABOVE : s.pos_of[v]));
        CHECK(ghosts);
        CHECK(NP_BELOW == -2 && NP_ABOVE == -3);
    }
}

static void check_slab_rules()
{
    g_case = "slab rules";
    // a slab per plane up to the cap, thicker slabs beyond it; a forced thickness never goes below what the cap needs
    Levels lv;
    lv.lmin = 3;
    lv.lmax = 40;
    CHECK(slab_cap(256, 1) == 192 && slab_cap(256, 2) == 96 && slab_cap(32, 1) == 24 && slab_cap(1, 4) == 1);
    SlabParams p = slab_params(5, 104, lv, 192, Forced());
    CHECK(p.dz == 1 && p.n_slabs == 100 && p.nl == 38 && p.zmin == 5 && p.lmin == 3);
    p = slab_params(0, 199, lv, 24, Forced());
    CHECK(p.dz == 9 && p.n_slabs == 23);
    p = slab_params(0, 199, lv, 24, forced(2));
    CHECK(p.dz == 9);
    p = slab_params(0, 199, lv, 24, forced(20));
    CHECK(p.dz == 20 && p.n_slabs == 10);
    CHECK(p.usable(3) && !p.usable(4));
    // a run longer than the sweep kernel's LDS holds: refused, nothing left behind
    const Volume big = make_volume("full 200x200x64", 200, 200, 64, 1.0, 0);
    const Owned own(big.coords.data(), big.V, 0, big.V);
    const HostThreads th(own.n(), forced(4));
    SlabNumbering s;
    CHECK(!number_slabs(own, scan_levels(own, 1, 1, th), 1, Forced(), 3, th, p, s));
    CHECK(p.n_slabs == 1 && s.pos_of.empty() && s.level_pos.empty() && s.level_count.empty() && s.sl_max_run == 0);
    CHECK(number_slabs(own, scan_levels(own, 1, 1, th), 192, Forced(), 3, th, p, s));
    CHECK(p.n_slabs == 64 && s.sl_max_run == 200 && slab_accepted(s, p, 192) && !slab_accepted(s, p, 63));
    // lanes per run
    CHECK(slab_width(10, Forced()) == 64 && slab_width(64, Forced()) == 64 && slab_width(65, Forced()) == 128);
    CHECK(slab_width(200, Forced()) == 256 && slab_width(5000, Forced()) == 1024);
    CHECK(slab_width(10, forced(256)) == 256 && slab_width(10, forced(192)) == 64 && slab_width(10, forced(100)) == 64);
    CHECK(slab_width(10, forced(4096)) == 1024 && slab_width(10, forced(0)) == 64);
    // the prep kernel's tiles: a full box takes them, a mask that fills little of its box does not
    PrepTiles t = prep_tiles(16, 16, 2, 5, 1024);
    CHECK(t.tile_nx == 2 && t.tile_ny == 2 && t.tile_z0 == 2 && t.n_tiles == 16);
    t = prep_tiles(800, 800, 0, 0, 100);
    CHECK(t.n_tiles == 0 && t.tile_nx == 0);
    // host threads: one below 2^18 items, never more than items
    CHECK(HostThreads(1000, Forced()).nt == 1 && HostThreads(3, forced(7)).nt == 3 && HostThreads(0, forced(7)).nt == 1);
    CHECK(HostThreads(1000, forced(1000)).nt == 64 && HostThreads(1000, forced(0)).nt == 1);
    const HostThreads h7(100, forced(7));
    CHECK(h7.chunk(0) == 0 && h7.chunk(7) == 100);
}

// ---- a_K segments ----
static void check_segments(const Volume &vol, int begin, int end)
{
    g_case = vol.name + " segments [" + std::to_string(begin) + "," + std::to_string(end) + ")";
    const Owned own(vol.coords.data(), vol.V, begin, end);
    const std::vector<int32_t> seg = ak_segments(own);
    CHECK(!seg.empty() && seg.back() == end);
    if (own.n() == 0)
        return;
    CHECK(seg.front() == begin);
    std::set<int32_t> starts(seg.begin(), seg.end());
    bool ok = true;
    for (size_t i = 0; i + 1 < seg.size(); i++)
    {
        ok = ok && seg[i] < seg[i + 1] && seg[i + 1] - seg[i] <= 4096;
        ok = ok && vol.Z()[seg[i]] == vol.Z()[seg[i + 1] - 1]; // within one plane
    }
    for (int v = begin + 1; v < end; v++)
        if (vol.Z()[v] != vol.Z()[v - 1])
            ok = ok && starts.count(v) == 1; // every plane starts a segment
    CHECK(ok);
}

// ---- the z-slabs of a run on several devices ----
static void check_slab_cuts(const Volume &vol)
{
    const int32_t *Z = vol.Z();
    std::vector<int> plane_start;
    g_case = vol.name + " planes";
    CHECK(plane_starts(Z, vol.V, plane_start));
    const int n_planes = (int)plane_start.size();
    for (int world = 1; world <= 4; world++)
        for (int halo = 1; halo <= 2; halo++)
        {
            g_case = vol.name + " slab cuts world=" + std::to_string(world) + " halo=" + std::to_string(halo);
            const std::vector<SlabCut> cuts = slab_cuts(Z, vol.V, plane_start, world, halo);
            const int n = (int)cuts.size();
            CHECK(n >= 1 && n <= world);
            CHECK(n == 1 || n <= n_planes / (2 * halo));
            CHECK(cuts.front().b == 0 && cuts.back().e == vol.V && cuts.front().g0 == 0 && cuts.back().g1 == vol.V);
            int want_halo = 1;
            for (int r = 0; r < n; r++)
            {
                const SlabCut &c = cuts[r];
                CHECK(c.b < c.e && c.g0 <= c.b && c.e <= c.g1);
                CHECK(c.b == 0 || Z[c.b] != Z[c.b - 1]); // on a plane boundary
                if (r + 1 < n)
                    CHECK(c.e == cuts[r + 1].b);
                std::set<int> planes(Z + c.b, Z + c.e);
                CHECK(n == 1 || (int)planes.size() >= halo);
                if (r > 0) // the ghosts below: the planes within `halo` of the lowest owned plane, all of the previous slab's
                {
                    CHECK(c.g0 >= cuts[r - 1].b);
                    CHECK(Z[c.g0] >= Z[c.b] - halo && (c.g0 == 0 || Z[c.g0 - 1] < Z[c.b] - halo));
                }
                if (r + 1 < n)
                {
                    CHECK(c.g1 <= cuts[r + 1].e);
                    CHECK(Z[c.g1 - 1] <= Z[c.e - 1] + halo && (c.g1 == vol.V || Z[c.g1] > Z[c.e - 1] + halo));
                }
                want_halo = std::max(want_halo, std::max(c.b - c.g0, c.g1 - c.e));
            }
            CHECK(max_halo(cuts) == want_halo);
        }
}

int main()
{
    std::vector<Volume> volumes;
    volumes.push_back(make_volume("masked 13x11x9", 13, 11, 9, 0.8, 1));
    volumes.push_back(make_volume("masked 24x7x16", 24, 7, 16, 0.8, 2));
    volumes.push_back(make_volume("full 8x9x10", 8, 9, 10, 1.0, 0));
    volumes.push_back(make_volume("planes missing", 10, 9, 14, 0.8, 3, { 3, 4, 9 }));
    volumes.push_back(make_volume("one plane", 12, 10, 1, 0.8, 4));
    for (const Volume &vol : volumes)
    {
        check_neighbours(vol);
        check_slab_cuts(vol);
        // the whole list, and a slab of it with ghost planes either side
        std::vector<int> plane_start;
        plane_starts(vol.Z(), vol.V, plane_start);
        std::vector<std::pair<int, int> > ranges(1, std::make_pair(0, vol.V));
        if (plane_start.size() >= 5)
            ranges.push_back(std::make_pair(plane_start[2], plane_start[plane_start.size() - 2]));
        for (const auto &r : ranges)
        {
            check_level_order(vol, r.first, r.second);
            check_slab_numbering(vol, r.first, r.second);
            check_segments(vol, r.first, r.second);
        }
    }
    {
        // a geometry the dense offset map does not take (the binary search of the reference)
        Volume sparse = make_volume("sparse box", 6, 5, 4, 0.8, 5);
        std::vector<int32_t> c;
        for (int dim = 0; dim < 3; dim++)
        {
            c.insert(c.end(), sparse.coords.begin() + (size_t)dim * sparse.V, sparse.coords.begin() + (size_t)(dim + 1) * sparse.V);
            c.push_back(dim == 2 ? 5000 : 299);
        }
        sparse.coords = c;
        sparse.V++;
        check_neighbours(sparse);
    }
    {
        // planes of more than 4096 voxels
        const Volume wide = make_volume("full 80x80x3", 80, 80, 3, 1.0, 0);
        check_segments(wide, 0, wide.V);
        check_segments(wide, 6400, 12800);
        check_slab_cuts(wide);
    }
    {
        // decompositions that do not go round: fewer slabs, finally one
        g_case = "slab cuts fall back";
        std::vector<int> ps;
        const Volume five = make_volume("five planes", 6, 6, 5, 0.8, 6);
        plane_starts(five.Z(), five.V, ps);
        CHECK(slab_cuts(five.Z(), five.V, ps, 4, 1).size() == 2);
        CHECK(slab_cuts(five.Z(), five.V, ps, 4, 2).size() == 1);
        const Volume three = make_volume("three planes", 6, 6, 3, 0.8, 7);
        plane_starts(three.Z(), three.V, ps);
        const std::vector<SlabCut> one = slab_cuts(three.Z(), three.V, ps, 4, 2);
        CHECK(one.size() == 1 && one[0].g0 == 0 && one[0].b == 0 && one[0].e == three.V && one[0].g1 == three.V);
        CHECK(slab_cuts(three.Z(), three.V, ps, 4, 1).size() == 1);
        // an unbalanced mask: nearly everything in the top plane
        Volume heavy = make_volume("heavy top", 4, 4, 6, 0.8, 8);
        const Volume top = make_volume("top", 40, 40, 1, 0.9, 9);
        std::vector<int32_t> c;
        for (int dim = 0; dim < 3; dim++)
        {
            c.insert(c.end(), heavy.coords.begin() + (size_t)dim * heavy.V, heavy.coords.begin() + (size_t)(dim + 1) * heavy.V);
            for (int v = 0; v < top.V; v++)
                c.push_back(dim == 2 ? 6 : top.coords[(size_t)dim * top.V + v]);
        }
        heavy.coords = c;
        heavy.V += top.V;
        heavy.name = "heavy top";
        check_slab_cuts(heavy);
        // z going down is refused
        std::vector<int32_t> z = { 0, 0, 1, 0 };
        CHECK(!plane_starts(z.data(), 4, ps));
    }
    check_slab_rules();
    printf("%d checks, %d failed\n", g_checks, g_failures);
    if (g_failures == 0)
        printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
