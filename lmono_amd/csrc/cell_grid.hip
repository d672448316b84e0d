// cell_grid.hip -- the cell grid under the outlier filter (sor.hip), the ICP's target (icp.hip) and the surface normals (normals.hip): how the
// neighbours of a point are found.  The points of a cloud are sorted into cells of side h keyed by vm_key: a hash table of the occupied cells (open
// addressing over a power of two >= 2 n of 64-bit keys, as the voxel map's), each with the count of its points and where they begin in `sorted`.
// A stage's job begins with a CellView `g`; every kernel takes blockIdx.y = stream over the stage's job table; none waits on another workgroup.
//
// A build is four launches, five with an origin:
//   k_cellgrid_clear    empties the cell table and resets the grid's words.  Alone it builds an empty grid.
//   k_cellgrid_minmax   (origin) min and max of the valid points per axis: integer atomics on the icp_ord keys, exact in any order.
//   k_cellgrid_cells    (origin: the origin from those words, the same bits on every thread;) per point validity, (span) and key; the cell is
//                       claimed with a 64-bit compare-and-swap, one atomic add on the cell's count gives the point its rank in the cell.
//   k_cellgrid_offsets  a prefix over the occupied cells in whatever order the workgroups arrive (one atomic per workgroup); with a work list
//                       also one item per kCellQ points of a cell, by a second sum in the upper half of the scanned word.
//   k_cellgrid_scatter  copies xyz + input index cell by cell.  The order inside a cell and the order of the cells differ from run to run;
//                       nothing downstream depends on them: neighbours are selected by value and every sum is an integer.
// Loop bounds: a probe is at most the table's size; the counts of a finished table sum to the placed points, and a cell's offset + count stays
// at or below that sum, which is at most n.
// The host side (CellGrid, cellgrid_slots, cellgrid_build) is at the end; it is written against lmono_hip.hip's lmono_ctx and check_launch.
#pragma once
#include "common.hpp"
#include "colour.hip"
#include "cell_grid.hpp"
#include "dev_owner.hpp"

namespace lmono {

constexpr int kCellT = 256;               // threads of the build kernels
constexpr int kCellQ = 64;                // points of a cell that share an item of the work list
constexpr unsigned kCellNoSlot = 0xffffffffu;

struct CellPt { float x, y, z; unsigned i; };      // a point of `sorted`: its index in the input cloud rides along
struct CellWork { unsigned slot, tile; };          // points tile * kCellQ ... of the cell at `slot`

// the words of a grid
struct CellWords {
    unsigned omin[3], omax[3];             // icp_ord keys over the valid points (origin pass)
    unsigned rejected, alloc;              // points invalid or out of span; points placed by k_cellgrid_offsets
    float o[3];                            // the origin; 0 without the origin pass
    unsigned nwork;                        // items of the work list
};

struct CellView {
    const PtRgb *pts;                      // the input cloud
    long long n;
    unsigned long long *key;               // the cell table: key, points, first point in `sorted`
    unsigned *cnt, *off;
    unsigned mask;                         // slots of this cloud - 1
    unsigned *slot, *rank;                 // per input point: its cell's slot (kCellNoSlot: rejected) and its rank in the cell
    CellPt *sorted;                        // the placed points cell by cell
    CellWork *work;                        // the work list, nullptr: none is written
    float h, inv;
    int rings;
    CellWords *w;
};

static_assert(sizeof(CellPt) == 16 && sizeof(CellWork) == 8 && sizeof(CellWords) % 8 == 0, "grid layouts");

// exclusive prefix of x over the T threads of a workgroup (wsum: T / 64 words of LDS); total = the workgroup's sum
template <int T> __device__ inline unsigned long long cellgrid_block_scan(unsigned long long x, unsigned long long *wsum, unsigned long long &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long incl = x;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    unsigned long long base = 0;
    total = 0;
    for (int u = 0; u < T / 64; u++) { if (u < w) base += wsum[u]; total += wsum[u]; }
    __syncthreads();                        // wsum may be written again
    return base + incl - x;
}

// slot of `key`, claimed if new.  The table has at least 2 n slots for at most n keys: the probe always ends early
__device__ inline unsigned cellgrid_claim(const CellView &g, uint64_t key)
{
    unsigned h = (unsigned)vm_mix(key) & g.mask;
    for (unsigned probe = 0; probe <= g.mask; probe++, h = (h + 1) & g.mask) {
        unsigned long long k = __hip_atomic_load(&g.key[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kVmEmpty) k = atomicCAS(&g.key[h], (unsigned long long)kVmEmpty, (unsigned long long)key);
        if (k == kVmEmpty || k == key) return h;
    }
    return kCellNoSlot;
}

// slot of `key` in the finished table, kCellNoSlot when no point lies in that cell
__device__ inline unsigned cellgrid_find(const CellView &g, uint64_t key)
{
    unsigned h = (unsigned)vm_mix(key) & g.mask;
    for (unsigned probe = 0; probe <= g.mask; probe++, h = (h + 1) & g.mask) {
        const unsigned long long k = g.key[h];
        if (k == key) return h;
        if (k == kVmEmpty) return kCellNoSlot;
    }
    return kCellNoSlot;
}

template <typename Job> __global__ __launch_bounds__(kCellT) void k_cellgrid_clear(const Job *jobs)
{
    const CellView &g = jobs[blockIdx.y].g;
    const unsigned long long s = (unsigned long long)blockIdx.x * kCellT + threadIdx.x;
    if (s == 0) {
        CellWords w;
        for (int a = 0; a < 3; a++) { w.omin[a] = 0xffffffffu; w.omax[a] = 0u; w.o[a] = 0.0f; }
        w.rejected = 0; w.alloc = 0; w.nwork = 0;
        *g.w = w;
    }
    if (s > g.mask) return;
    g.key[s] = kVmEmpty;
    g.cnt[s] = 0;
}

template <typename Job> __global__ __launch_bounds__(kCellT) void k_cellgrid_minmax(const Job *jobs)
{
    const CellView &g = jobs[blockIdx.y].g;
    const long long i = (long long)blockIdx.x * kCellT + threadIdx.x;
    if ((long long)blockIdx.x * kCellT >= g.n) return;
    __shared__ unsigned l_min[3], l_max[3];
    if (threadIdx.x < 3) { l_min[threadIdx.x] = 0xffffffffu; l_max[threadIdx.x] = 0u; }
    __syncthreads();
    if (i < g.n) {
        const PtRgb pt = g.pts[i];
        uint64_t key;
        int c[3];
        if (sor_cell(pt.x, pt.y, pt.z, g.inv, key, c)) {
            const unsigned k[3] = { icp_ord(pt.x), icp_ord(pt.y), icp_ord(pt.z) };
            for (int a = 0; a < 3; a++) { atomicMin(&l_min[a], k[a]); atomicMax(&l_max[a], k[a]); }
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 && l_min[threadIdx.x] <= l_max[threadIdx.x]) {
        atomicMin(&g.w->omin[threadIdx.x], l_min[threadIdx.x]);
        atomicMax(&g.w->omax[threadIdx.x], l_max[threadIdx.x]);
    }
}

// kOrigin: the origin from the min / max words (0 when no point is valid) is written to the words, and a valid point out of span is rejected
template <typename Job, bool kOrigin> __global__ __launch_bounds__(kCellT) void k_cellgrid_cells(const Job *jobs)
{
    const CellView &g = jobs[blockIdx.y].g;
    const long long i = (long long)blockIdx.x * kCellT + threadIdx.x;
    if ((long long)blockIdx.x * kCellT >= g.n) return;
    __shared__ unsigned l_rej;
    if (threadIdx.x == 0) l_rej = 0;
    __syncthreads();
    float o[3] = { 0.0f, 0.0f, 0.0f };
    if constexpr (kOrigin) {
        for (int a = 0; a < 3; a++) {
            const unsigned mn = g.w->omin[a], mx = g.w->omax[a];
            if (mn <= mx) o[a] = icp_origin(icp_unord(mn), icp_unord(mx));
        }
        if (i == 0) for (int a = 0; a < 3; a++) g.w->o[a] = o[a];
    }
    if (i < g.n) {
        const PtRgb pt = g.pts[i];
        uint64_t key = kVmEmpty;
        int c[3];
        unsigned slot = kCellNoSlot;
        bool ok = sor_cell(pt.x, pt.y, pt.z, g.inv, key, c);
        if constexpr (kOrigin) ok = ok && icp_in_span(pt.x - o[0]) && icp_in_span(pt.y - o[1]) && icp_in_span(pt.z - o[2]);
        if (ok) slot = cellgrid_claim(g, key);
        g.slot[i] = slot;
        if (slot == kCellNoSlot) atomicAdd(&l_rej, 1u);
        else g.rank[i] = atomicAdd(&g.cnt[slot], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && l_rej) atomicAdd(&g.w->rejected, l_rej);
}

template <typename Job> __global__ __launch_bounds__(kCellT) void k_cellgrid_offsets(const Job *jobs)
{
    const CellView &g = jobs[blockIdx.y].g;
    const unsigned long long s = (unsigned long long)blockIdx.x * kCellT + threadIdx.x;
    if (g.n == 0 || (unsigned long long)blockIdx.x * kCellT > g.mask) return;
    __shared__ unsigned long long wsum[kCellT / 64], l_base;
    const unsigned c = s <= g.mask ? g.cnt[s] : 0u;
    const unsigned t = g.work ? (c + kCellQ - 1) / kCellQ : 0u;
    unsigned long long total;
    const unsigned long long ex = cellgrid_block_scan<kCellT>((unsigned long long)t << 32 | c, wsum, total);      // both sums stay below 2^32: n <= 2^28
    if (threadIdx.x == 0 && total) {
        const unsigned bc = atomicAdd(&g.w->alloc, (unsigned)total);
        const unsigned bt = g.work ? atomicAdd(&g.w->nwork, (unsigned)(total >> 32)) : 0u;
        l_base = (unsigned long long)bt << 32 | bc;
    }
    __syncthreads();
    if (c == 0) return;
    const unsigned long long at = l_base + ex;          // no carry between the halves: each half is a sum below 2^32
    g.off[s] = (unsigned)at;
    for (unsigned q = 0; q < t; q++) { CellWork &w = g.work[(at >> 32) + q]; w.slot = (unsigned)s; w.tile = q; }
}

template <typename Job> __global__ __launch_bounds__(kCellT) void k_cellgrid_scatter(const Job *jobs)
{
    const CellView &g = jobs[blockIdx.y].g;
    const long long i = (long long)blockIdx.x * kCellT + threadIdx.x;
    if (i >= g.n) return;
    const unsigned slot = g.slot[i];
    if (slot == kCellNoSlot) return;
    const PtRgb pt = g.pts[i];
    CellPt p;
    p.x = pt.x; p.y = pt.y; p.z = pt.z; p.i = (unsigned)i;
    g.sorted[g.off[slot] + g.rank[i]] = p;              // below the number of placed points, which is at most n
}

} // namespace lmono

// ---- the host side: what a handle owns of its grid

// slots of the grid of n points: the smallest power of two >= 2 n, at least 64
static uint64_t cellgrid_slots(int64_t n)
{
    uint64_t slots = 64;
    while (slots < 2 * (uint64_t)n) slots <<= 1;
    return slots;
}

struct CellGrid {
    float h = 0.0f, inv = 0.0f;
    int rings = 0;
    uint64_t slots = 0;                      // of the allocation; a call uses cellgrid_slots(n) of them
    unsigned long long *key = nullptr;
    unsigned *cnt = nullptr, *off = nullptr, *slot = nullptr, *rank = nullptr;
    lmono::CellPt *sorted = nullptr;
    lmono::CellWork *work = nullptr;
    lmono::CellWords *words = nullptr;

    bool alloc(DevOwner &mem, int64_t max_points, float cell, int max_rings, bool work_list)
    {
        h = cell; inv = 1.0f / cell; rings = max_rings;
        slots = cellgrid_slots(max_points);
        const size_t n = (size_t)max_points;
        return mem.alloc(key, (size_t)slots) && mem.alloc(cnt, (size_t)slots) && mem.alloc(off, (size_t)slots) && mem.alloc(slot, n) && mem.alloc(rank, n) &&
               mem.alloc(sorted, n) && (!work_list || mem.alloc(work, n + n / lmono::kCellQ + 1)) && mem.alloc_zero(words, 1);
    }
    // the view of a cloud of n points (n <= max_points, so cellgrid_slots(n) <= slots)
    lmono::CellView view(const lmono::PtRgb *pts, int64_t n) const
    {
        lmono::CellView g;
        g.pts = pts; g.n = n;
        g.key = key; g.cnt = cnt; g.off = off; g.mask = (unsigned)(cellgrid_slots(n) - 1);
        g.slot = slot; g.rank = rank; g.sorted = sorted; g.work = work;
        g.h = h; g.inv = inv; g.rings = rings; g.w = words;
        return g;
    }
};

// The build of the grids of a job table (n streams, Job::g; max_n: the largest g.n) on c's stream: one launch per phase for all streams.
// kOrigin: the min / max pass runs and the cells apply origin and span.  max_n == 0: the clear alone, which leaves every grid empty.
template <bool kOrigin, typename Job> static int cellgrid_build(lmono_ctx *c, const Job *jobs, int n, int64_t max_n)
{
    using namespace lmono;
    const dim3 g_slots((unsigned)((cellgrid_slots(max_n) + kCellT - 1) / kCellT), (unsigned)n), g_pts((unsigned)((max_n + kCellT - 1) / kCellT), (unsigned)n);
    k_cellgrid_clear<<<g_slots, kCellT, 0, c->stream>>>(jobs);
    if (int rc = check_launch(c, "k_cellgrid_clear")) return rc;
    if (max_n == 0) return LMONO_OK;
    if constexpr (kOrigin) {
        k_cellgrid_minmax<<<g_pts, kCellT, 0, c->stream>>>(jobs);
        if (int rc = check_launch(c, "k_cellgrid_minmax")) return rc;
    }
    k_cellgrid_cells<Job, kOrigin><<<g_pts, kCellT, 0, c->stream>>>(jobs);
    if (int rc = check_launch(c, "k_cellgrid_cells")) return rc;
    k_cellgrid_offsets<<<g_slots, kCellT, 0, c->stream>>>(jobs);
    if (int rc = check_launch(c, "k_cellgrid_offsets")) return rc;
    k_cellgrid_scatter<<<g_pts, kCellT, 0, c->stream>>>(jobs);
    return check_launch(c, "k_cellgrid_scatter");
}
