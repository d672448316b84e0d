// track_reject.hip -- FeatureTracker::rejectWithF (FeatureTracker.cc:259-262, :435-503) on the device: DESIGN.md 6e item 4a.
// Two epipolar gates on the survivors of the forward-backward test: a fixed number of 8-point hypotheses from a counter-based
// sample stream, scored in fp64 (gate 1), a least-squares refit over the winner's inliers (what cv::findFundamentalMat returns)
// and the symmetric distance test of :467-499 against that F (gate 2).  Every step is one IEEE fp64 operation in the order
// written here and in tests/track_reject_ref.py (the library is built with -ffp-contract=off), so the two agree bit for bit.
// The arithmetic (rej_*) is plain C++ and also compiles for the host; k_trk_reject below is included by track.hip.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define REJ_HD __host__ __device__ __forceinline__
#else
#define REJ_HD inline
#endif

namespace lmono {

constexpr int kRejT = 256;            // threads of the workgroup
constexpr int kRejChunk = 64;         // hypotheses solved at a time, one per lane of wave 0, their 8 x 9 systems in LDS
constexpr int kRejMaxHyp = 1024;
constexpr int kRejMaxDraws = 256;     // draws of one sample before the hypothesis is given up as invalid
constexpr int kRejSweeps = 7;         // cyclic Jacobi sweeps (the measured residue)
constexpr int kRejPts = 512;          // LMONO_TRACK_MAX_POINTS
constexpr double kRejSqrt2 = 1.4142135623730951;

REJ_HD uint32_t rej_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// key of hypothesis h of the frame; draw d of its sample is rej_mix(key ^ d)
REJ_HD uint32_t rej_key(uint32_t seed, uint32_t frame, uint32_t h) { return rej_mix(rej_mix(rej_mix(seed ^ 0x9e3779b9u) ^ frame) ^ h); }

REJ_HD bool rej_sample(uint32_t key, int m, int *idx)
{
    int d = 0;
#pragma unroll
    for (int jj = 0; jj < 8; jj++) {
        int v = -1;
        while (d < kRejMaxDraws) {
            const uint32_t r = rej_mix(key ^ (uint32_t)d);
            d++;
            const int c = (int)(((uint64_t)r * (uint64_t)(uint32_t)m) >> 32);
            bool dup = false;
#pragma unroll
            for (int q = 0; q < 8; q++) dup = dup || (q < jj && idx[q] == c);
            if (!dup) { v = c; break; }
        }
        if (v < 0) return false;
        idx[jj] = v;
    }
    return true;
}

// the virtual-camera point as gate 1 sees it: rounded once to fp32 (cv::Point2f)
REJ_HD double rej_g1(double v) { return (double)(float)v; }

// F = Tp^T Fn Tc for the normalisations p^ = (p - mp) sp, c^ = (c - mc) sc
REJ_HD void rej_denorm(const double *Fn, double sp, double mpx, double mpy, double sc, double mcx, double mcy, double *F)
{
    const double tp0 = -(mpx * sp), tp1 = -(mpy * sp), tc0 = -(mcx * sc), tc1 = -(mcy * sc);
    double G[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        G[3 * i] = Fn[3 * i] * sc;
        G[3 * i + 1] = Fn[3 * i + 1] * sc;
        G[3 * i + 2] = (Fn[3 * i] * tc0 + Fn[3 * i + 1] * tc1) + Fn[3 * i + 2];
    }
#pragma unroll
    for (int jj = 0; jj < 3; jj++) {
        F[jj] = sp * G[jj];
        F[3 + jj] = sp * G[3 + jj];
        F[6 + jj] = (tp0 * G[jj] + tp1 * G[3 + jj]) + G[6 + jj];
    }
}

// element i of (a, b, 1): a row of the 8-point system is (px, py, 1) (x) (cx, cy, 1), and a product with 1.0 is exact
REJ_HD double rej_pick(int i, double a, double b) { return i == 0 ? a : (i == 1 ? b : 1.0); }

// r^2 of prev^T F cur and the squared norms of the two epipolar lines l = F cur, l' = F^T prev
REJ_HD void rej_epi(const double *F, double px, double py, double cx, double cy, double &r2, double &lc, double &lp)
{
    const double l0 = (F[0] * cx + F[1] * cy) + F[2], l1 = (F[3] * cx + F[4] * cy) + F[5], l2 = (F[6] * cx + F[7] * cy) + F[8];
    const double r = (px * l0 + py * l1) + l2;
    const double m0 = (F[0] * px + F[3] * py) + F[6], m1 = (F[1] * px + F[4] * py) + F[7];
    r2 = r * r; lc = l0 * l0 + l1 * l1; lp = m0 * m0 + m1 * m1;
}
REJ_HD bool rej_inlier(const double *F, double px, double py, double cx, double cy, double thr2)
{
    double r2, lc, lp;
    rej_epi(F, px, py, cx, cy, r2, lc, lp);
    return (r2 / lc <= thr2) && (r2 / lp <= thr2);       // max(e, e') <= thr2; a NaN (0 / 0) is no inlier
}

// One minimal solve.  pd: [4][kRejPts] virtual-camera points (prev X, prev Y, cur X, cur Y) in fp64; A: the 8 x 9 system, element
// (r, c) at A[(r * 9 + c) * S]; x: 9 values at x[e * S] (the null vector, then F row-major).  S is the lane stride of the LDS image.
template <int S> REJ_HD bool rej_solve(const double *pd, int m, uint32_t key, double *A, double *x)
{
    int idx[8];
    if (!rej_sample(key, m, idx)) return false;
    double mpx = 0.0, mpy = 0.0, mcx = 0.0, mcy = 0.0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        mpx = mpx + rej_g1(pd[idx[k]]); mpy = mpy + rej_g1(pd[kRejPts + idx[k]]);
        mcx = mcx + rej_g1(pd[2 * kRejPts + idx[k]]); mcy = mcy + rej_g1(pd[3 * kRejPts + idx[k]]);
    }
    mpx = mpx / 8.0; mpy = mpy / 8.0; mcx = mcx / 8.0; mcy = mcy / 8.0;
    double dp = 0.0, dc = 0.0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const double ax = rej_g1(pd[idx[k]]) - mpx, ay = rej_g1(pd[kRejPts + idx[k]]) - mpy;
        const double bx = rej_g1(pd[2 * kRejPts + idx[k]]) - mcx, by = rej_g1(pd[3 * kRejPts + idx[k]]) - mcy;
        dp = dp + sqrt(ax * ax + ay * ay); dc = dc + sqrt(bx * bx + by * by);
    }
    dp = dp / 8.0; dc = dc / 8.0;
    if (!(dp > 0.0) || !(dc > 0.0)) return false;
    const double sp = kRejSqrt2 / dp, sc = kRejSqrt2 / dc;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const double a = (rej_g1(pd[idx[k]]) - mpx) * sp, b = (rej_g1(pd[kRejPts + idx[k]]) - mpy) * sp;
        const double c = (rej_g1(pd[2 * kRejPts + idx[k]]) - mcx) * sc, d = (rej_g1(pd[3 * kRejPts + idx[k]]) - mcy) * sc;
        double *row = A + (size_t)(k * 9) * S;
        row[0] = a * c; row[S] = a * d; row[2 * S] = a; row[3 * S] = b * c; row[4 * S] = b * d; row[5 * S] = b;
        row[6 * S] = c; row[7 * S] = d; row[8 * S] = 1.0;
    }
    // Gaussian elimination with complete pivoting: rows and columns are marked, not swapped
    unsigned row_used = 0u, col_used = 0u, prs = 0u, pcs = 0u;
    for (int k = 0; k < 8; k++) {
        double best = -1.0;
        int pr = -1, pc = -1;
        for (int r = 0; r < 8; r++) {
            if (row_used >> r & 1u) continue;
            for (int c = 0; c < 9; c++) {
                if (col_used >> c & 1u) continue;
                const double v = fabs(A[(size_t)(r * 9 + c) * S]);
                if (v > best) { best = v; pr = r; pc = c; }
            }
        }
        if (!(best >= 1e-12)) return false;
        const double piv = A[(size_t)(pr * 9 + pc) * S];
        row_used |= 1u << pr; col_used |= 1u << pc;
        prs |= (unsigned)pr << (3 * k); pcs |= (unsigned)pc << (4 * k);
        for (int r = 0; r < 8; r++) {
            if (row_used >> r & 1u) continue;
            const double f = A[(size_t)(r * 9 + pc) * S] / piv;
            for (int c = 0; c < 9; c++) {
                if (col_used >> c & 1u) continue;
                A[(size_t)(r * 9 + c) * S] = A[(size_t)(r * 9 + c) * S] - f * A[(size_t)(pr * 9 + c) * S];
            }
        }
    }
    int cf = 0;
    for (int c = 0; c < 9; c++) if (!(col_used >> c & 1u)) cf = c;
    x[(size_t)cf * S] = 1.0;
    for (int k = 7; k >= 0; k--) {
        const int pr = (int)(prs >> (3 * k) & 7u), pc = (int)(pcs >> (4 * k) & 15u);
        double acc = A[(size_t)(pr * 9 + cf) * S];
        for (int q = k + 1; q < 8; q++) {
            const int c = (int)(pcs >> (4 * q) & 15u);
            acc = acc + A[(size_t)(pr * 9 + c) * S] * x[(size_t)c * S];
        }
        x[(size_t)pc * S] = -acc / A[(size_t)(pr * 9 + pc) * S];
    }
    double Fn[9], F[9];
#pragma unroll
    for (int e = 0; e < 9; e++) Fn[e] = x[(size_t)e * S];
    rej_denorm(Fn, sp, mpx, mpy, sc, mcx, mcy, F);
#pragma unroll
    for (int e = 0; e < 9; e++) x[(size_t)e * S] = F[e];
    return true;
}

// cyclic Jacobi on the symmetric N x N matrix A (both triangles kept), V = the rotations' product; fixed sweeps, fixed (p, q) order
template <int N> REJ_HD void rej_jacobi(double *A, double *V, int sweeps)
{
    for (int i = 0; i < N * N; i++) V[i] = (i / N == i % N) ? 1.0 : 0.0;
    for (int s = 0; s < sweeps; s++)
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++) {
                const double apq = A[p * N + q];
                if (apq == 0.0) continue;
                const double app = A[p * N + p], aqq = A[q * N + q];
                const double theta = (aqq - app) / (2.0 * apq);
                double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < N; k++) {
                    if (k == p || k == q) continue;
                    const double akp = A[k * N + p], akq = A[k * N + q];
                    const double n1 = c * akp - sn * akq, n2 = sn * akp + c * akq;
                    A[k * N + p] = n1; A[p * N + k] = n1; A[k * N + q] = n2; A[q * N + k] = n2;
                }
                A[p * N + p] = app - t * apq; A[q * N + q] = aqq + t * apq;
                A[p * N + q] = 0.0; A[q * N + p] = 0.0;
                for (int k = 0; k < N; k++) {
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = c * vkp - sn * vkq; V[k * N + q] = sn * vkp + c * vkq;
                }
            }
}
template <int N> REJ_HD int rej_smallest(const double *A)
{
    int b = 0;
    for (int i = 1; i < N; i++) if (A[i * N + i] < A[b * N + b]) b = i;
    return b;
}

// M (9 x 9, both triangles) -> the refit F: smallest eigenvector, rank 2 by deflation, denormalised.  V, G, V3: work space (81, 9, 9)
REJ_HD void rej_refit(double *M, double *V, double *G, double *V3, double sp, double mpx, double mpy, double sc, double mcx, double mcy, double *F)
{
    rej_jacobi<9>(M, V, kRejSweeps);
    const int b = rej_smallest<9>(M);
    double Fn[9];
#pragma unroll
    for (int e = 0; e < 9; e++) Fn[e] = V[e * 9 + b];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int c = a; c < 3; c++) {
            const double g = (Fn[a] * Fn[c] + Fn[3 + a] * Fn[3 + c]) + Fn[6 + a] * Fn[6 + c];
            G[a * 3 + c] = g; G[c * 3 + a] = g;
        }
    rej_jacobi<3>(G, V3, kRejSweeps);
    const int b3 = rej_smallest<3>(G);
    const double v0 = V3[b3], v1 = V3[3 + b3], v2 = V3[6 + b3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double w = (Fn[3 * i] * v0 + Fn[3 * i + 1] * v1) + Fn[3 * i + 2] * v2;
        Fn[3 * i] = Fn[3 * i] - w * v0; Fn[3 * i + 1] = Fn[3 * i + 1] - w * v1; Fn[3 * i + 2] = Fn[3 * i + 2] - w * v2;
    }
    rej_denorm(Fn, sp, mpx, mpy, sc, mcx, mcy, F);
}

#if defined(__HIPCC__)

// PINHOLE liftProjective in fp64 (the 8 rounds of trk_lift, not rounded) onto the virtual camera of :441-453
__device__ __forceinline__ void rej_lift(const ColourCam &c, float2 p, double focal, double &X, double &Y)
{
    const double mx_d = c.ik11 * (double)p.x + c.ik13, my_d = c.ik22 * (double)p.y + c.ik23;
    double mx_u = mx_d, my_u = my_d;
    if (c.distort) {
        for (int it = 0; it < 8; it++) {
            double dx, dy;
            col_distortion(c, mx_u, my_u, dx, dy);
            mx_u = mx_d - dx; my_u = my_d - dy;
        }
    }
    X = focal * mx_u + (double)c.w / 2.0;
    Y = focal * my_u + (double)c.h / 2.0;
}

// One workgroup per stream, between the backward k_trk_lk and k_trk_update; a stream without rejection leaves at once.
// Writes one status byte per point slot (1: survives the :226-243 tests and both gates), stats [4] and F [9].
__global__ __launch_bounds__(kRejT) void k_trk_reject(const TrkJob *jobs)
{
    __shared__ double s_A[72 * kRejChunk], s_x[9 * kRejChunk], s_pd[4 * kRejPts];
    __shared__ double s_M[81], s_V[81], s_G[9], s_V3[9], s_F[9], s_nrm[6];
    __shared__ unsigned long long s_best;
    __shared__ int s_cnt[kRejChunk], s_valid[kRejChunk], s_m, s_nvalid, s_kept;
    __shared__ unsigned short s_idx[kRejPts];
    __shared__ unsigned char s_flag[kRejPts], s_out[kRejPts];
    const TrkJob &j = jobs[blockIdx.x];
    if (!j.rej_st) return;
    const int tid = threadIdx.x;
    const bool diag = j.rej_n >= 0;
    const int n = min(max(diag ? j.rej_n : j.st->n, 0), kRejPts);
    for (int i = tid; i < kRejPts; i += kRejT) { s_flag[i] = (i < n && (diag || trk_keep(j, i))) ? 1 : 0; s_out[i] = 0; }
    if (tid == 0) s_kept = 0;
    __syncthreads();
    {   // the survivors in order (:245-248)
        const int i0 = tid, i1 = tid + kRejT;
        int r0 = 0, r1 = 0, tot = 0;
        for (int k = 0; k < n; k++) { const int f = s_flag[k]; tot += f; r0 += k < i0 ? f : 0; r1 += k < i1 ? f : 0; }
        if (i0 < n && s_flag[i0]) s_idx[r0] = (unsigned short)i0;
        if (i1 < n && s_flag[i1]) s_idx[r1] = (unsigned short)i1;
        if (tid == 0) s_m = tot;
    }
    __syncthreads();
    const int m = s_m;
    if (m < 8) {        // :437 -- the step does not run
        for (int i = tid; i < n; i += kRejT) j.rej_st[i] = s_flag[i];
        if (tid < 4) j.rej_stats[tid] = -1;
        if (tid < 9) j.rej_F[tid] = 0.0;
        return;
    }
    for (int k = tid; k < m; k += kRejT) {
        const int slot = s_idx[k];
        const float2 p = diag ? j.rej_prev[slot] : j.pts[slot], c = diag ? j.rej_cur[slot] : j.cur_pts[slot];
        double X, Y;
        rej_lift(j.cam, p, j.rej_focal, X, Y); s_pd[k] = X; s_pd[kRejPts + k] = Y;
        rej_lift(j.cam, c, j.rej_focal, X, Y); s_pd[2 * kRejPts + k] = X; s_pd[3 * kRejPts + k] = Y;
    }
    __syncthreads();
    // hypotheses, kRejChunk at a time: wave 0 solves one per lane, then all four waves score them, a quarter of the points each
    const int nh = min(j.rej_nhyp, kRejMaxHyp);
    const double thr2 = j.rej_thr2;
    unsigned long long best = 0ull;
    int nvalid = 0;
    for (int h0 = 0; h0 < nh; h0 += kRejChunk) {
        if (tid < kRejChunk) {
            s_cnt[tid] = 0;
            const int h = h0 + tid;
            s_valid[tid] = (h < nh && rej_solve<kRejChunk>(s_pd, m, rej_key(j.rej_seed, j.rej_key, (uint32_t)h), s_A + tid, s_x + tid)) ? 1 : 0;
        }
        __syncthreads();
        {
            const int hl = tid & (kRejChunk - 1), part = tid / kRejChunk;
            if (s_valid[hl]) {
                double F[9];
#pragma unroll
                for (int e = 0; e < 9; e++) F[e] = s_x[e * kRejChunk + hl];
                int cnt = 0;
                for (int i = part; i < m; i += kRejT / kRejChunk)
                    cnt += rej_inlier(F, rej_g1(s_pd[i]), rej_g1(s_pd[kRejPts + i]), rej_g1(s_pd[2 * kRejPts + i]), rej_g1(s_pd[3 * kRejPts + i]), thr2) ? 1 : 0;
                atomicAdd(&s_cnt[hl], cnt);
            }
        }
        __syncthreads();
        if (tid < kRejChunk && s_valid[tid]) {      // larger key: more inliers, then the lower h
            nvalid++;
            const unsigned long long key = ((unsigned long long)(unsigned int)s_cnt[tid] << 32) | (0xFFFFFFFFu - (unsigned int)(h0 + tid));
            best = key > best ? key : best;
        }
    }
    if (tid < kWave) {
        best = wave_max_key_uniform(best);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nvalid += __shfl_xor(nvalid, o);
        if (tid == 0) { s_best = best; s_nvalid = nvalid; }
    }
    __syncthreads();
    const unsigned long long bk = s_best;
    const int bcnt = (int)(bk >> 32), bh = bk ? (int)(0xFFFFFFFFu - (unsigned int)bk) : -1;
    if (bk == 0ull || bcnt < 8) {       // OpenCV's zero mask at :458-461: every survivor is dropped
        for (int i = tid; i < n; i += kRejT) j.rej_st[i] = 0;
        if (tid == 0) { j.rej_stats[0] = s_nvalid; j.rej_stats[1] = bh; j.rej_stats[2] = bcnt; j.rej_stats[3] = 0; }
        if (tid < 9) j.rej_F[tid] = 0.0;
        return;
    }
    if (tid == 0) {
        rej_solve<kRejChunk>(s_pd, m, rej_key(j.rej_seed, j.rej_key, (uint32_t)bh), s_A, s_x);
        for (int e = 0; e < 9; e++) s_F[e] = s_x[e * kRejChunk];
    }
    __syncthreads();
    for (int k = tid; k < m; k += kRejT)
        s_flag[k] = rej_inlier(s_F, rej_g1(s_pd[k]), rej_g1(s_pd[kRejPts + k]), rej_g1(s_pd[2 * kRejPts + k]), rej_g1(s_pd[3 * kRejPts + k]), thr2) ? 1 : 0;
    __syncthreads();
    // refit over the gate-1 inliers: every sum runs over ascending point index in one thread
    if (tid < 4) {
        double acc = 0.0; int cnt = 0;
        for (int k = 0; k < m; k++) if (s_flag[k]) { acc = acc + rej_g1(s_pd[tid * kRejPts + k]); cnt++; }
        s_nrm[tid] = acc / (double)cnt;
    }
    __syncthreads();
    if (tid < 2) {
        const double mx = s_nrm[2 * tid], my = s_nrm[2 * tid + 1];
        double acc = 0.0; int cnt = 0;
        for (int k = 0; k < m; k++) if (s_flag[k]) {
            const double ax = rej_g1(s_pd[2 * tid * kRejPts + k]) - mx, ay = rej_g1(s_pd[(2 * tid + 1) * kRejPts + k]) - my;
            acc = acc + sqrt(ax * ax + ay * ay); cnt++;
        }
        s_nrm[4 + tid] = acc / (double)cnt;
    }
    __syncthreads();
    const double mpx = s_nrm[0], mpy = s_nrm[1], mcx = s_nrm[2], mcy = s_nrm[3], dp = s_nrm[4], dc = s_nrm[5];
    if (!(dp > 0.0) || !(dc > 0.0)) {   // the inliers coincide in one image: no F, every survivor is dropped
        for (int i = tid; i < n; i += kRejT) j.rej_st[i] = 0;
        if (tid == 0) { j.rej_stats[0] = s_nvalid; j.rej_stats[1] = bh; j.rej_stats[2] = bcnt; j.rej_stats[3] = 0; }
        if (tid < 9) j.rej_F[tid] = 0.0;
        return;
    }
    const double sp = kRejSqrt2 / dp, sc = kRejSqrt2 / dc;
    if (tid < 45) {     // entry (a, b), a <= b, of M = A^T A
        int a = 0, rem = tid;
        while (rem >= 9 - a) { rem -= 9 - a; a++; }
        const int b = a + rem;
        double acc = 0.0;
        for (int k = 0; k < m; k++) if (s_flag[k]) {
            const double l0 = (rej_g1(s_pd[k]) - mpx) * sp, l1 = (rej_g1(s_pd[kRejPts + k]) - mpy) * sp;
            const double r0 = (rej_g1(s_pd[2 * kRejPts + k]) - mcx) * sc, r1 = (rej_g1(s_pd[3 * kRejPts + k]) - mcy) * sc;
            acc = acc + (rej_pick(a / 3, l0, l1) * rej_pick(a % 3, r0, r1)) * (rej_pick(b / 3, l0, l1) * rej_pick(b % 3, r0, r1));
        }
        s_M[a * 9 + b] = acc; s_M[b * 9 + a] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        rej_refit(s_M, s_V, s_G, s_V3, sp, mpx, mpy, sc, mcx, mcy, s_F);
        for (int e = 0; e < 9; e++) j.rej_F[e] = s_F[e];
    }
    __syncthreads();
    // gate 2 (:467-499) on the gate-1 inliers, with the unrounded points
    int kept = 0;
    for (int k = tid; k < m; k += kRejT) {
        if (!s_flag[k]) continue;
        double r2, lc, lp;
        rej_epi(s_F, s_pd[k], s_pd[kRejPts + k], s_pd[2 * kRejPts + k], s_pd[3 * kRejPts + k], r2, lc, lp);
        const double s = r2 / (lc + lp);
        if (!(s > j.rej_dis)) { s_out[s_idx[k]] = 1; kept++; }
    }
    if (kept) atomicAdd(&s_kept, kept);
    __syncthreads();
    for (int i = tid; i < n; i += kRejT) j.rej_st[i] = s_out[i];
    if (tid == 0) { j.rej_stats[0] = s_nvalid; j.rej_stats[1] = bh; j.rej_stats[2] = bcnt; j.rej_stats[3] = s_kept; }
}

#endif // __HIPCC__

} // namespace lmono
