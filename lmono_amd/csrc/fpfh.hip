// fpfh.hip -- FPFH descriptors at keypoints on gfx950: the pcl::FPFHEstimation with a search surface of
// MapBuilder::alignmentToMap (Map_Builder.cc:110-210), as a device-resident stage behind the surface normals.  The arithmetic is fpfh.hpp; this
// file is how the neighbours are found and where the histograms live.  Every kernel takes blockIdx.y = stream over an array of jobs; none waits on
// another workgroup.
//
// The grid over the surface is a grid with an origin (cell_grid.hip), built by this stage with its own cell, so that the radius is independent of
// the normals'.  Then
//   k_fpfh_clear    the per-point words of the needed list and the stream's device words.
//   k_fpfh_mark     one wave per keypoint: every point with a normal within r of it is claimed once (a compare-and-swap on its word) and appended to
//                   the list of needed points.  The order of the list differs from run to run; a point's SPFH does not depend on its row.
//   k_fpfh_spfh     the hot kernel: one needed point per thread.  k_nrm_compute's neighbour loop; each pair's three bins are counted in the
//                   thread's own column of an LDS array [33][kFpfhT]: a histogram indexed by a computed bin would leave the registers, and the
//                   columns are conflict-free (consecutive lanes, consecutive banks).  The row of 33 counts and the pair count goes to HBM.
//   k_fpfh_weight   one wave per keypoint: the lanes share the points of each cell, each keeps 66 integer partial sums in registers (every index
//                   static), a butterfly of shuffles adds them, lane 0 turns them into fp64 values in LDS and 33 lanes scale one bin each.
// The stream's stats are integer atomics at the end of k_fpfh_spfh and k_fpfh_weight (sums and maxima: exact in any order), not a launch of their own.
// Loop bounds: the rings are at most max_rings, the points of a cell its count; the grid's own are at the head of cell_grid.hip.  The list holds
// at most one entry per point with a normal, so at most g.n.
#pragma once
#include "cell_grid.hip"
#include "fpfh.hpp"

namespace lmono {

constexpr int kFpfhT = 128;                // threads of k_fpfh_spfh: 33 * 128 * 4 = 16.5 KB of LDS per workgroup
constexpr int kFpfhMarkT = 256;            // four keypoints per workgroup of k_fpfh_mark

// what a compute keeps per stream on the device: needed points, sum and largest of their pair counts, keypoints with and without a
// descriptor, sum and largest of the keypoints' contributing neighbours
struct FpfhDev { unsigned long long w[8]; };

struct FpfhJob {
    CellView g;                            // the surface and its grid
    const NrmRecord *rec;                  // the surface's records
    const float *kp;                       // [m][3]
    int m;
    float r2;
    unsigned *need;                        // per point: 0, or 1 + its row in list / spfh
    unsigned *list;                        // the needed points
    unsigned *spfh;                        // [needed][kFpfhRow]
    float *desc;                           // [m][33]
    unsigned *nb, *flag;                   // [m]
    FpfhDev *dev;
};

__global__ __launch_bounds__(kCellT) void k_fpfh_clear(const FpfhJob *jobs)
{
    const FpfhJob &q = jobs[blockIdx.y];
    const long long i = (long long)blockIdx.x * kCellT + threadIdx.x;
    if (i == 0) for (int w = 0; w < 8; w++) q.dev->w[w] = 0;
    if (i < q.g.n) q.need[i] = 0;
}

__global__ __launch_bounds__(kFpfhMarkT) void k_fpfh_mark(const FpfhJob *jobs)
{
    const FpfhJob &q = jobs[blockIdx.y];
    const CellView &g = q.g;
    const int k = blockIdx.x * (kFpfhMarkT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= q.m || g.n == 0) return;
    const float kx = q.kp[3 * k], ky = q.kp[3 * k + 1], kz = q.kp[3 * k + 2];
    uint64_t key;
    int c[3];
    if (!sor_cell(kx, ky, kz, g.inv, key, c)) return;
    constexpr int L = 1 << 20;
    const int R = g.rings;
    for (int dz = -R; dz <= R; dz++)
        for (int dy = -R; dy <= R; dy++)
            for (int dx = -R; dx <= R; dx++) {
                const int x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
                if (x < -L || x >= L || y < -L || y >= L || z < -L || z >= L) continue;
                const unsigned slot = cellgrid_find(g, vm_key(x, y, z));
                if (slot == kCellNoSlot) continue;
                const unsigned n = g.cnt[slot];
                const CellPt *p = g.sorted + g.off[slot];
                for (unsigned e = lane; e < n; e += 64) {
                    const CellPt m = p[e];
                    if (!(sor_d2(kx, ky, kz, m.x, m.y, m.z) <= q.r2) || !fpfh_has_normal(q.rec[m.i].nx)) continue;
                    if (atomicCAS(&q.need[m.i], 0u, 1u) != 0u) continue;                     // another keypoint claimed it
                    const unsigned row = (unsigned)atomicAdd(&q.dev->w[0], 1ull);           // below the points with a normal, at most g.n
                    q.list[row] = m.i;
                    q.need[m.i] = row + 1;                                                   // read by the launches after this one
                }
            }
}

__global__ __launch_bounds__(kFpfhT) void k_fpfh_spfh(const FpfhJob *jobs)
{
    const FpfhJob &q = jobs[blockIdx.y];
    const CellView &g = q.g;
    const unsigned long long needed = q.dev->w[0];
    if ((unsigned long long)blockIdx.x * kFpfhT >= needed) return;
    __shared__ unsigned l_h[kFpfhDim][kFpfhT];
    const unsigned long long t = (unsigned long long)blockIdx.x * kFpfhT + threadIdx.x;
    const int tid = threadIdx.x;
#pragma unroll
    for (int b = 0; b < kFpfhDim; b++) l_h[b][tid] = 0;              // the thread's own column: no barrier
    unsigned pairs = 0;
    if (t < needed) {
        const unsigned i = q.list[t];
        const PtRgb pt = g.pts[i];
        const NrmRecord ni = q.rec[i];
        uint64_t key;
        int c[3];
        sor_cell(pt.x, pt.y, pt.z, g.inv, key, c);
        constexpr int L = 1 << 20;
        const int R = g.rings;
        for (int dz = -R; dz <= R; dz++)
            for (int dy = -R; dy <= R; dy++)
                for (int dx = -R; dx <= R; dx++) {
                    const int x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
                    if (x < -L || x >= L || y < -L || y >= L || z < -L || z >= L) continue;
                    const unsigned slot = cellgrid_find(g, vm_key(x, y, z));
                    if (slot == kCellNoSlot) continue;
                    const unsigned n = g.cnt[slot];
                    const CellPt *p = g.sorted + g.off[slot];
                    for (unsigned e = 0; e < n; e++) {
                        const CellPt m = p[e];
                        const float d2 = sor_d2(pt.x, pt.y, pt.z, m.x, m.y, m.z);
                        if (!(d2 > 0.0f && d2 <= q.r2)) continue;
                        const NrmRecord nj = q.rec[m.i];
                        if (!fpfh_has_normal(nj.nx)) continue;
                        int b[3];
                        if (!fpfh_pair(pt.x, pt.y, pt.z, ni.nx, ni.ny, ni.nz, m.x, m.y, m.z, nj.nx, nj.ny, nj.nz, b)) continue;
                        l_h[b[0]][tid] += 1; l_h[kFpfhBins + b[1]][tid] += 1; l_h[2 * kFpfhBins + b[2]][tid] += 1;
                        pairs++;
                    }
                }
        unsigned *row = q.spfh + t * kFpfhRow;
#pragma unroll
        for (int b = 0; b < kFpfhDim; b++) row[b] = l_h[b][tid];
        row[kFpfhDim] = pairs;
    }
    unsigned long long sum = pairs, big = pairs;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_xor(sum, d);
        const unsigned long long other = __shfl_xor(big, d);
        if (other > big) big = other;
    }
    if ((threadIdx.x & 63) == 0 && sum) { atomicAdd(&q.dev->w[1], sum); atomicMax(&q.dev->w[2], big); }
}

__global__ __launch_bounds__(64) void k_fpfh_weight(const FpfhJob *jobs)
{
    const FpfhJob &q = jobs[blockIdx.y];
    const CellView &g = q.g;
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= q.m) return;
    __shared__ double l_v[kFpfhDim];
    uint64_t hi[kFpfhDim], lo[kFpfhDim];
#pragma unroll
    for (int b = 0; b < kFpfhDim; b++) { hi[b] = 0; lo[b] = 0; }
    unsigned nb = 0;
    const float kx = q.kp[3 * k], ky = q.kp[3 * k + 1], kz = q.kp[3 * k + 2];
    uint64_t key;
    int c[3];
    if (g.n > 0 && sor_cell(kx, ky, kz, g.inv, key, c)) {
        constexpr int L = 1 << 20;
        const int R = g.rings;
        for (int dz = -R; dz <= R; dz++)
            for (int dy = -R; dy <= R; dy++)
                for (int dx = -R; dx <= R; dx++) {
                    const int x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
                    if (x < -L || x >= L || y < -L || y >= L || z < -L || z >= L) continue;
                    const unsigned slot = cellgrid_find(g, vm_key(x, y, z));
                    if (slot == kCellNoSlot) continue;
                    const unsigned n = g.cnt[slot];
                    const CellPt *p = g.sorted + g.off[slot];
                    for (unsigned e = lane; e < n; e += 64) {
                        const CellPt m = p[e];
                        const float d2 = sor_d2(kx, ky, kz, m.x, m.y, m.z);
                        if (!(d2 <= q.r2)) continue;
                        const unsigned at = q.need[m.i];
                        if (at == 0) continue;                                  // without a normal
                        const unsigned *row = q.spfh + (unsigned long long)(at - 1) * kFpfhRow;
                        const unsigned nj = row[kFpfhDim];
                        if (nj == 0) continue;
                        const uint64_t W = fpfh_weight(d2, nj);
                        nb++;
#pragma unroll
                        for (int b = 0; b < kFpfhDim; b++) fpfh_add(W, row[b], hi[b], lo[b]);
                    }
                }
    }
#pragma unroll 1
    for (int d = 32; d > 0; d >>= 1) {                                          // rolled: six copies of 66 shuffles double the registers
#pragma unroll
        for (int b = 0; b < kFpfhDim; b++) {
            hi[b] += (uint64_t)__shfl_xor((unsigned long long)hi[b], d);
            lo[b] += (uint64_t)__shfl_xor((unsigned long long)lo[b], d);
        }
        nb += __shfl_xor(nb, d);
    }
    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < kFpfhDim; b++) l_v[b] = fpfh_value(hi[b], lo[b]);
    }
    __syncthreads();
    if (lane < kFpfhDim) q.desc[(long long)k * kFpfhDim + lane] = nb ? fpfh_scale(l_v[lane], fpfh_total(l_v + (lane / kFpfhBins) * kFpfhBins)) : 0.0f;
    if (lane == 0) {
        q.nb[k] = nb;
        q.flag[k] = nb ? 1u : 0u;
        atomicAdd(&q.dev->w[nb ? 3 : 4], 1ull);
        if (nb) { atomicAdd(&q.dev->w[5], (unsigned long long)nb); atomicMax(&q.dev->w[6], (unsigned long long)nb); }
    }
}

} // namespace lmono
