// icp.hip -- point-to-point ICP of a frame cloud against a target cloud on gfx950: the pcl::IterativeClosestPoint that
// MapBuilder::processMapping carries commented out between its outlier removal and its voxel grid (Map_Builder.cc:31-59), as a device-resident
// stage between the outlier filter and the voxel map.  The arithmetic is icp.hpp; this file is how the neighbours are found and the sums formed.
// Every kernel takes blockIdx.y = stream over an array of jobs; none waits on another workgroup.
//
// A target is the grid of the target cloud, with an origin (cell_grid.hip); it is built once and serves every align until the next one.
// An align is k_icp_prepare, then max_iter pairs of k_icp_step and k_icp_solve, then k_icp_apply:
//   k_icp_prepare   guess, u and the usable flag per source point.
//   k_icp_step      the hot kernel: one source point per thread.  q under the stream's state, its cell, then ring by ring the cells of Chebyshev
//                   distance r (ring 1 with the cell itself) through L2, keeping the best pair by icp_better, until the best d2 <= sor_rho2(r, h) or
//                   r = max_rings.  The 26 words of an accepted pair are summed over the wave with shuffles, over the workgroup in LDS, and added
//                   with 64-bit atomics into the sum words of the iteration's parity.
//   k_icp_solve     lane 0 of one workgroup per stream: icp_iterate on the sums, history[k], the done word, and the clear of the other parity's
//                   sums (those of the next iteration).
//   k_icp_apply     the aligned cloud under the final state.
// k_icp_step and k_icp_solve return at once for a stream whose done word is set, so the result does not depend on how many pairs the host enqueues.
#pragma once
#include "cell_grid.hip"
#include "icp.hpp"

namespace lmono {

constexpr int kIcpT = 256;                // threads of every kernel here but k_icp_solve

struct IcpU { float x, y, z; unsigned usable; };

// what an align keeps per stream on the device
struct IcpDev {
    IcpState st;
    IcpSums sums[2];                       // of the iterations of either parity
    unsigned long long unusable;
};

struct IcpJob {
    CellView g;                            // the target
    float D2;
    // source
    const PtRgb *pts;
    long long n;
    IcpU *u;
    float *d2;
    PtRgb *out;
    IcpDev *dev;
    long long *hist;                       // [max_iter][2]
    int *done;
    int max_iter;
    double eps, mse_eps;
    double G[12];
};

static_assert(sizeof(IcpU) == 16, "icp layouts");

__global__ __launch_bounds__(kIcpT) void k_icp_prepare(const IcpJob *jobs)
{
    const IcpJob &j = jobs[blockIdx.y];
    const long long i = (long long)blockIdx.x * kIcpT + threadIdx.x;
    if ((long long)blockIdx.x * kIcpT >= j.n) return;
    __shared__ unsigned l_bad;
    if (threadIdx.x == 0) l_bad = 0;
    __syncthreads();
    if (i < j.n) {
        const PtRgb pt = j.pts[i];
        const float *o = j.g.w->o;
        IcpU u;
        u.x = icp_guess_axis(j.G, pt.x, pt.y, pt.z) - o[0];
        u.y = icp_guess_axis(j.G + 4, pt.x, pt.y, pt.z) - o[1];
        u.z = icp_guess_axis(j.G + 8, pt.x, pt.y, pt.z) - o[2];
        u.usable = icp_in_span(u.x) && icp_in_span(u.y) && icp_in_span(u.z) ? 1u : 0u;
        j.u[i] = u;
        j.d2[i] = INFINITY;
        if (!u.usable) atomicAdd(&l_bad, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && l_bad) atomicAdd(&j.dev->unusable, (unsigned long long)l_bad);
}

__global__ __launch_bounds__(kIcpT) void k_icp_step(const IcpJob *jobs)
{
    const IcpJob &j = jobs[blockIdx.y];
    const long long i = (long long)blockIdx.x * kIcpT + threadIdx.x;
    if ((long long)blockIdx.x * kIcpT >= j.n || *j.done) return;
    __shared__ long long l_sum[kIcpT / 64][kIcpWords];
    const IcpState &st = j.dev->st;
    const int par = (st.k + 1) & 1;
    long long s[kIcpWords];
#pragma unroll
    for (int w = 0; w < kIcpWords; w++) s[w] = 0;
    bool acc = false;
    if (i < j.n) {
        const IcpU u = j.u[i];
        float best = INFINITY, bx = 0.0f, by = 0.0f, bz = 0.0f;
        const float *o = j.g.w->o;
        const float o0 = o[0], o1 = o[1], o2 = o[2];
        uint64_t key;
        int c[3];
        if (u.usable) {
            const float qx = icp_q_axis(st.R, st.tau[0], o0, u.x, u.y, u.z), qy = icp_q_axis(st.R + 3, st.tau[1], o1, u.x, u.y, u.z),
                        qz = icp_q_axis(st.R + 6, st.tau[2], o2, u.x, u.y, u.z);
            if (sor_cell(qx, qy, qz, j.g.inv, key, c)) {
                constexpr int L = 1 << 20;
                for (int r = 1; r <= j.g.rings; r++) {
                    for (int dz = -r; dz <= r; dz++)
                        for (int dy = -r; dy <= r; dy++)
                            for (int dx = -r; dx <= r; dx++) {
                                if (r > 1 && abs(dx) < r && abs(dy) < r && abs(dz) < r) continue;      // inside: seen at the rings before
                                const int x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
                                if (x < -L || x >= L || y < -L || y >= L || z < -L || z >= L) continue;
                                const unsigned slot = cellgrid_find(j.g, vm_key(x, y, z));
                                if (slot == kCellNoSlot) continue;
                                const unsigned n = j.g.cnt[slot];
                                const CellPt *p = j.g.sorted + j.g.off[slot];
                                for (unsigned e = 0; e < n; e++) {
                                    const CellPt m = p[e];
                                    const float d2 = sor_d2(qx, qy, qz, m.x, m.y, m.z);
                                    if (icp_better(d2, m.x, m.y, m.z, best, bx, by, bz)) { best = d2; bx = m.x; by = m.y; bz = m.z; }
                                }
                            }
                    if (best <= sor_rho2(r, j.g.h)) break;
                }
                acc = best <= j.D2;
            }
        }
        j.d2[i] = acc ? best : INFINITY;
        if (acc) {
            const float uu[3] = { u.x, u.y, u.z }, ww[3] = { bx - o0, by - o1, bz - o2 };
            IcpSums t;
            icp_terms(uu, ww, best, t);
            s[0] = t.N; s[25] = t.E;
#pragma unroll
            for (int a = 0; a < 3; a++) { s[1 + a] = t.Su[a]; s[4 + a] = t.Sw[a]; }
#pragma unroll
            for (int e = 0; e < 9; e++) { s[7 + e] = t.hi[e]; s[16 + e] = t.lo[e]; }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (__any(acc)) {
#pragma unroll
        for (int w = 0; w < kIcpWords; w++)
            for (int d = 32; d > 0; d >>= 1) s[w] += __shfl_xor(s[w], d);
    }
    if (lane == 0) {
#pragma unroll
        for (int w = 0; w < kIcpWords; w++) l_sum[wave][w] = s[w];
    }
    __syncthreads();
    if (threadIdx.x < kIcpWords) {
        long long n = 0, v = 0;
        for (int w = 0; w < kIcpT / 64; w++) { n += l_sum[w][0]; v += l_sum[w][threadIdx.x]; }
        if (n) atomicAdd((unsigned long long *)&j.dev->sums[par] + threadIdx.x, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(64) void k_icp_solve(const IcpJob *jobs)
{
    const IcpJob &j = jobs[blockIdx.y];
    if (threadIdx.x != 0 || *j.done) return;
    IcpState st = j.dev->st;
    const int par = (st.k + 1) & 1;
    const IcpSums s = j.dev->sums[par];
    icp_iterate(st, s, j.max_iter, j.eps, j.mse_eps);
    j.hist[2 * (long long)(st.k - 1)] = s.N;            // st.k <= max_iter: a stream is done at max_iter at the latest
    j.hist[2 * (long long)(st.k - 1) + 1] = s.E;
    j.dev->st = st;
    long long *next = (long long *)&j.dev->sums[par ^ 1];
    for (int w = 0; w < kIcpWords; w++) next[w] = 0;
    *j.done = st.done;
}

__global__ __launch_bounds__(kIcpT) void k_icp_apply(const IcpJob *jobs)
{
    const IcpJob &j = jobs[blockIdx.y];
    const long long i = (long long)blockIdx.x * kIcpT + threadIdx.x;
    if (i >= j.n) return;
    const IcpState &st = j.dev->st;
    const IcpU u = j.u[i];
    const float *o = j.g.w->o;
    PtRgb p = j.pts[i];
    p.x = icp_q_axis(st.R, st.tau[0], o[0], u.x, u.y, u.z);
    p.y = icp_q_axis(st.R + 3, st.tau[1], o[1], u.x, u.y, u.z);
    p.z = icp_q_axis(st.R + 6, st.tau[2], o[2], u.x, u.y, u.z);
    j.out[i] = p;
}

} // namespace lmono
