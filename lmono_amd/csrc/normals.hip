// normals.hip -- surface normals and curvature of a cloud on gfx950: the pcl::NormalEstimation that opens
// MapBuilder::alignmentToMap (Map_Builder.cc:110-210), as a device-resident stage beside the outlier filter, the aligner and the voxel map.
// The arithmetic is normals.hpp; this file is how the neighbours are found.  Every kernel takes blockIdx.y = stream over an array of jobs;
// none waits on another workgroup.
//
// The grid over the cloud itself is a grid with an origin (cell_grid.hip): the validity, origin and span of the ICP's target.  Then
//   k_nrm_compute   the hot kernel: one point per thread.  Its cell, then every cell within ring R of it through L2 (cellgrid_find, the cell's count and
//                   offset, its points one by one); each point with d2 <= r * r adds its ten integer words in registers; the fp64 solve runs once
//                   from the finished words and the record and the count are written in input order.
//   k_nrm_stats     the count words of a stream reduced over the wave with shuffles, over the workgroup in LDS, then integer atomics.
// Loop bounds: the rings are at most max_rings, the points of a cell its count; the grid's own are at the head of cell_grid.hip.
#pragma once
#include "cell_grid.hip"
#include "normals.hpp"

namespace lmono {

constexpr int kNrmT = 256;

// what a compute keeps per stream on the device: rejected, with a normal, without, sum and largest of the counts
struct NrmDev { unsigned long long w[5]; };

struct NrmJob {
    CellView g;                            // the cloud and its grid
    NrmRecord *rec;
    unsigned *count;
    NrmDev *dev;
    float r2;
    int min_nb, has_vp;
    float vp[3];
};

__global__ __launch_bounds__(kNrmT) void k_nrm_compute(const NrmJob *jobs)
{
    const NrmJob &q = jobs[blockIdx.y];
    const CellView &g = q.g;
    const long long i = (long long)blockIdx.x * kNrmT + threadIdx.x;
    if (i == 0) for (int w = 0; w < 5; w++) q.dev->w[w] = 0;          // k_nrm_stats, the next launch, adds into them
    if (i >= g.n) return;
    NrmRecord out = nrm_no_normal();
    unsigned cnt = 0;
    if (g.slot[i] != kCellNoSlot) {                                      // placed by k_cellgrid_cells: valid and in span
        const PtRgb pt = g.pts[i];
        const float o0 = g.w->o[0], o1 = g.w->o[1], o2 = g.w->o[2];
        const int iw[3] = { nrm_fix(pt.x - o0), nrm_fix(pt.y - o1), nrm_fix(pt.z - o2) };
        uint64_t key;
        int c[3];
        sor_cell(pt.x, pt.y, pt.z, g.inv, key, c);
        NrmSums s;
        s.N = 0;
#pragma unroll
        for (int a = 0; a < 3; a++) s.S[a] = 0;
#pragma unroll
        for (int e = 0; e < 6; e++) s.SS[e] = 0;
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
                        if (!(sor_d2(pt.x, pt.y, pt.z, m.x, m.y, m.z) <= q.r2)) continue;
                        const int jw[3] = { nrm_fix(m.x - o0), nrm_fix(m.y - o1), nrm_fix(m.z - o2) };
                        nrm_add(iw, jw, s);
                    }
                }
        cnt = (unsigned)s.N;
        if (s.N >= q.min_nb) out = nrm_solve(s, pt.x, pt.y, pt.z, q.has_vp ? q.vp : nullptr);
    }
    q.rec[i] = out;
    q.count[i] = cnt;
}

__global__ __launch_bounds__(kNrmT) void k_nrm_stats(const NrmJob *jobs)
{
    const NrmJob &q = jobs[blockIdx.y];
    const CellView &g = q.g;
    const long long i = (long long)blockIdx.x * kNrmT + threadIdx.x;
    if ((long long)blockIdx.x * kNrmT >= g.n) return;
    __shared__ unsigned long long l_w[kNrmT / 64][5];
    unsigned long long w[5] = { 0, 0, 0, 0, 0 };
    if (i < g.n) {
        const unsigned n = q.count[i];
        w[0] = n == 0; w[1] = n >= (unsigned)q.min_nb; w[2] = n != 0 && n < (unsigned)q.min_nb; w[3] = n; w[4] = n;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] += __shfl_xor(w[k], d);
        const unsigned long long other = __shfl_xor(w[4], d);
        if (other > w[4]) w[4] = other;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) for (int k = 0; k < 5; k++) l_w[wave][k] = w[k];
    __syncthreads();
    if (threadIdx.x < 5) {
        unsigned long long v = 0;
        for (int g = 0; g < kNrmT / 64; g++) v = threadIdx.x < 4 ? v + l_w[g][threadIdx.x] : (l_w[g][4] > v ? l_w[g][4] : v);
        if (threadIdx.x < 4) { if (v) atomicAdd(&q.dev->w[threadIdx.x], v); }
        else atomicMax(&q.dev->w[4], v);
    }
}

} // namespace lmono
