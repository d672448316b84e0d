// sacia.hip -- the sample-consensus initial alignment on FPFH descriptors on gfx950: computeInitialAlignment of
// MapBuilder::alignmentToMap (Map_Builder.cc:110-210).  The arithmetic is sacia.hpp; this file is where the work runs.  No kernel waits on another
// workgroup; every loop is bounded by ns, nt <= 4096, K <= 32, kSaciaMaxDraws or the hypotheses of the launch.
//   k_sacia_cand   one wave per source entry: its nt descriptor distances go to LDS, then K rounds each take the least (D, j) after the one taken
//                  before it (a strided scan and a butterfly of shuffles): exact selection, ties to the lowest target index.
//   k_sacia_hyp    one workgroup per hypothesis.  Thread 0 draws the sample and the partners and fits (icp_solve) while the others stage the
//                  target keypoints in LDS (48 KB at 4096); then every thread takes source entries, searches all targets for the nearest one and
//                  adds its truncated term and inlier to the workgroup's integer sums in LDS.  Hypotheses may be split over launches: a
//                  hypothesis reads nothing another one wrote.
//   k_sacia_best   one workgroup: the least (error, h) over the hypotheses that are not void, and their number.
#pragma once
#include "sacia.hpp"

namespace lmono {

constexpr int kSaciaT = 256;

struct SaciaResult { unsigned long long err; int ok, h; unsigned inl, voids; };

struct SaciaJob {
    const float *sdesc, *tdesc;            // the descriptors of the two handles, [m][33], in keypoint order
    const int *sl, *tl;                    // the lists: keypoint index of every entry
    const float *u, *w, *tpos;             // [ns][3] centred source, [nt][3] centred target, [nt][3] target positions
    int ns, nt, K, n_hyp;
    uint32_t seed;
    float msd2, mc2, ct[3];
    int *cand;                             // [ns][K] target entries
    unsigned long long *err;               // [n_hyp]
    unsigned *inl;                         // [n_hyp]
    double *fit;                           // [n_hyp][12]: R, tau
    SaciaResult *res;
};

__global__ __launch_bounds__(64) void k_sacia_cand(SaciaJob q)
{
    __shared__ float l_d[kFpfhMaxKeypoints];
    __shared__ float l_a[kFpfhDim];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= q.ns) return;
    if (lane < kFpfhDim) l_a[lane] = q.sdesc[(size_t)q.sl[i] * kFpfhDim + lane];
    __syncthreads();
    for (int j = lane; j < q.nt; j += 64) l_d[j] = sacia_desc_d2(l_a, q.tdesc + (size_t)q.tl[j] * kFpfhDim);
    __syncthreads();
    float pd = -1.0f;                      // the one taken before: distances are >= 0
    int pj = -1;
    for (int k = 0; k < q.K; k++) {
        float bd = INFINITY;
        int bj = q.nt;
        for (int j = lane; j < q.nt; j += 64) {
            const float d = l_d[j];
            if (sacia_before(pd, pj, d, j) && sacia_before(d, j, bd, bj)) { bd = d; bj = j; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(bd, off);
            const int oj = __shfl_xor(bj, off);
            if (sacia_before(od, oj, bd, bj)) { bd = od; bj = oj; }
        }
        if (lane == 0) q.cand[(size_t)i * q.K + k] = bj < q.nt ? bj : q.nt - 1;      // K <= nt finite distances: bj < nt
        pd = bd; pj = bj;
    }
}

__global__ __launch_bounds__(kSaciaT) void k_sacia_hyp(SaciaJob q, int h0)
{
    __shared__ float l_t[3 * kFpfhMaxKeypoints];
    __shared__ double l_fit[12];
    __shared__ int l_ok;
    __shared__ unsigned long long l_err;
    __shared__ unsigned l_inl;
    const int h = h0 + blockIdx.x, tid = threadIdx.x;
    if (h >= q.n_hyp) return;
    if (tid == 0) {
        double R[9], tau[3];
        const bool ok = sacia_fit(pnp_key(q.seed, kSaciaKey, (uint32_t)h), q.ns, q.u, q.w, q.cand, q.K, q.msd2, R, tau);
        l_ok = ok ? 1 : 0; l_err = 0; l_inl = 0;
        if (ok) {
            for (int e = 0; e < 9; e++) l_fit[e] = R[e];
            for (int a = 0; a < 3; a++) l_fit[9 + a] = tau[a];
        }
    } else {
        for (int j = tid - 1; j < 3 * q.nt; j += kSaciaT - 1) l_t[j] = q.tpos[j];
    }
    __syncthreads();
    if (!l_ok) {                           // uniform for the workgroup
        if (tid == 0) { q.err[h] = kSaciaVoid; q.inl[h] = 0; }
        return;
    }
    double R[9], tau[3];
    for (int e = 0; e < 9; e++) R[e] = l_fit[e];
    for (int a = 0; a < 3; a++) tau[a] = l_fit[9 + a];
    unsigned long long e_sum = 0;
    unsigned inl = 0;
    for (int i = tid; i < q.ns; i += kSaciaT) {
        const float ux = q.u[3 * i], uy = q.u[3 * i + 1], uz = q.u[3 * i + 2];
        const float qx = icp_q_axis(R, tau[0], q.ct[0], ux, uy, uz), qy = icp_q_axis(R + 3, tau[1], q.ct[1], ux, uy, uz), qz = icp_q_axis(R + 6, tau[2], q.ct[2], ux, uy, uz);
        float best = INFINITY;
        for (int j = 0; j < q.nt; j++) {
            const float d2 = sor_d2(qx, qy, qz, l_t[3 * j], l_t[3 * j + 1], l_t[3 * j + 2]);
            if (d2 < best) best = d2;
        }
        e_sum += sacia_term(best, q.mc2);
        inl += best <= q.mc2 ? 1u : 0u;
    }
    atomicAdd(&l_err, e_sum);
    atomicAdd(&l_inl, inl);
    __syncthreads();
    if (tid == 0) {
        q.err[h] = l_err; q.inl[h] = l_inl;
        for (int e = 0; e < 12; e++) q.fit[(size_t)h * 12 + e] = l_fit[e];
    }
}

__global__ __launch_bounds__(kSaciaT) void k_sacia_best(SaciaJob q)
{
    __shared__ unsigned long long l_e[kSaciaT];
    __shared__ int l_h[kSaciaT];
    __shared__ unsigned l_v[kSaciaT];
    const int tid = threadIdx.x;
    unsigned long long be = kSaciaVoid;
    int bh = q.n_hyp;
    unsigned voids = 0;
    for (int h = tid; h < q.n_hyp; h += kSaciaT) {
        const unsigned long long e = q.err[h];
        if (e == kSaciaVoid) { voids++; continue; }
        if (e < be || (e == be && h < bh)) { be = e; bh = h; }
    }
    l_e[tid] = be; l_h[tid] = bh; l_v[tid] = voids;
    __syncthreads();
    for (int s = kSaciaT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const unsigned long long e = l_e[tid + s];
            const int h = l_h[tid + s];
            if (h < q.n_hyp && (l_h[tid] >= q.n_hyp || e < l_e[tid] || (e == l_e[tid] && h < l_h[tid]))) { l_e[tid] = e; l_h[tid] = h; }
            l_v[tid] += l_v[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        SaciaResult r;
        r.ok = l_h[0] < q.n_hyp ? 1 : 0; r.h = r.ok ? l_h[0] : -1; r.err = r.ok ? l_e[0] : 0; r.inl = r.ok ? q.inl[l_h[0]] : 0; r.voids = l_v[0];
        *q.res = r;
    }
}

} // namespace lmono
