// pnp.hip -- KeyFrame::PnPRANSAC (KeyFrame.cc:296-351) on the device: DESIGN.md 6g.
// A fixed number of 4-point hypotheses from the counter-based sample stream of 6e item 4a, each a fixed number of damped Gauss-Newton
// steps from the caller's guess, scored in fp64 against every matched pair; the winner is refitted over its inliers by the same
// iteration, every sum in a fixed tree.  Every step is one IEEE fp64 operation in the order written here and in tests/pnp_ref.py
// (the library is built with -ffp-contract=off), so the two agree bit for bit.  The arithmetic (pnp_*) is plain C++ and also compiles
// for the host (lmono_amd/host/pnp_test.cpp runs pnp_ransac_host without a GPU); k_pnp_ransac below is included by pnp_abi.hip.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PNP_HD __host__ __device__ __forceinline__
#else
#define PNP_HD inline
#endif

namespace lmono {

constexpr int kPnpT = 256;            // threads of the workgroup
constexpr int kPnpPts = 512;          // LMONO_TRACK_MAX_POINTS
constexpr int kPnpMaxHyp = 1024;
constexpr int kPnpMaxDraws = 256;     // draws of one sample before the hypothesis is given up as invalid
constexpr int kPnpIters = 12;         // steps of every solve (the measured settling)
constexpr int kPnpDamp = 6;           // the first kPnpDamp steps are damped by lambda_k = 4^-k, the rest are plain Gauss-Newton
constexpr double kPnpPivot = 1e-12;   // a pivot of the 6 x 6 elimination below this: invalid
constexpr int kPnpC = 27;             // 21 entries of the upper triangle of H, row-major, then g [6]

PNP_HD uint32_t pnp_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// key of hypothesis h of the candidate `key`; draw d of its sample is pnp_mix(key ^ d)
PNP_HD uint32_t pnp_key(uint32_t seed, uint32_t key, uint32_t h) { return pnp_mix(pnp_mix(pnp_mix(seed ^ 0x9e3779b9u) ^ key) ^ h); }

PNP_HD bool pnp_sample(uint32_t key, int m, int *idx)
{
    int d = 0;
#pragma unroll
    for (int jj = 0; jj < 4; jj++) {
        int v = -1;
        while (d < kPnpMaxDraws) {
            const uint32_t r = pnp_mix(key ^ (uint32_t)d);
            d++;
            const int c = (int)(((uint64_t)r * (uint64_t)(uint32_t)m) >> 32);
            bool dup = false;
#pragma unroll
            for (int q = 0; q < 4; q++) dup = dup || (q < jj && idx[q] == c);
            if (!dup) { v = c; break; }
        }
        if (v < 0) return false;
        idx[jj] = v;
    }
    return true;
}

// a pose is t [3], q [4] (x y z w): camera from world
struct PnpPose { double t[3], q[4]; };

// Hamilton product a (x) b
PNP_HD void pnp_qmul(const double *a, const double *b, double *o)
{
    const double x = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    const double y = ((a[3] * b[1] - a[0] * b[2]) + a[1] * b[3]) + a[2] * b[0];
    const double z = ((a[3] * b[2] + a[0] * b[1]) - a[1] * b[0]) + a[2] * b[3];
    const double w = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
    o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}
PNP_HD void pnp_qnormalise(double *q)
{
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
}
// R(q), row-major
PNP_HD void pnp_rot(const double *q, double *R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz); R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz); R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy); R[7] = 2.0 * (yz + wx); R[8] = 1.0 - 2.0 * (xx + yy);
}
PNP_HD void pnp_apply(const double *R, const double *t, const double *X, double *p)
{
    p[0] = ((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + t[0];
    p[1] = ((R[3] * X[0] + R[4] * X[1]) + R[5] * X[2]) + t[1];
    p[2] = ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + t[2];
}

// the guess of :308-312 from the VIO pose (T_vio, q_vio) and the camera extrinsic (t_lc, q_lc), all t (x y z), q (x y z w)
PNP_HD void pnp_guess(const double *vio_tq, const double *ex_tq, PnpPose &g)
{
    double qwc[4], Rv[9], Rc[9], z[3] = { 0.0, 0.0, 0.0 }, twc[3], p[3];
    pnp_qmul(vio_tq + 3, ex_tq + 3, qwc);
    g.q[0] = -qwc[0]; g.q[1] = -qwc[1]; g.q[2] = -qwc[2]; g.q[3] = qwc[3];
    pnp_qnormalise(g.q);
    pnp_rot(vio_tq + 3, Rv);
    pnp_apply(Rv, vio_tq, ex_tq, twc);          // T_vio + R(q_vio) t_lc, summed as pnp_apply does
    pnp_rot(g.q, Rc);
    pnp_apply(Rc, z, twc, p);
    g.t[0] = -p[0]; g.t[1] = -p[1]; g.t[2] = -p[2];
}

PNP_HD bool pnp_inlier(const double *R, const double *t, const double *X, double u, double v, double thr2)
{
    double p[3];
    pnp_apply(R, t, X, p);
    const double dx = p[0] / p[2] - u, dy = p[1] / p[2] - v;
    return (p[2] > 0.0) && (dx * dx + dy * dy <= thr2);       // a NaN is no inlier
}

// One point's share of the normal equations, c [27]: H (upper triangle, row-major) then g, for the residual (p.x / p.z - u, p.y / p.z - v)
// and the step (dt, dtheta) of t += dt, q <- q (x) [dtheta / 2, 1].  false: p.z <= 0 (c is not written)
PNP_HD bool pnp_contrib(const double *R, const double *t, const double *X, double u, double v, double *c)
{
    double p[3];
    pnp_apply(R, t, X, p);
    if (!(p[2] > 0.0)) return false;
    const double iz = 1.0 / p[2], nx = p[0] / p[2], ny = p[1] / p[2], rx = nx - u, ry = ny - v, gx = nx * iz, gy = ny * iz;
    // dp / dtheta = -R [X]x, column k
    double D[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        D[3 * r] = R[3 * r + 2] * X[1] - R[3 * r + 1] * X[2];
        D[3 * r + 1] = R[3 * r] * X[2] - R[3 * r + 2] * X[0];
        D[3 * r + 2] = R[3 * r + 1] * X[0] - R[3 * r] * X[1];
    }
    double Jx[6], Jy[6];
    Jx[0] = iz; Jx[1] = 0.0; Jx[2] = -gx; Jy[0] = 0.0; Jy[1] = iz; Jy[2] = -gy;
#pragma unroll
    for (int k = 0; k < 3; k++) { Jx[3 + k] = iz * D[k] - gx * D[6 + k]; Jy[3 + k] = iz * D[3 + k] - gy * D[6 + k]; }
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++) c[e++] = Jx[a] * Jx[b] + Jy[a] * Jy[b];
#pragma unroll
    for (int a = 0; a < 6; a++) c[21 + a] = Jx[a] * rx + Jy[a] * ry;
    return true;
}

// (H + lam diag H) delta = -g by elimination in the natural order, the diagonal as pivots (no exchanges); s [27] is overwritten
PNP_HD bool pnp_solve6(double *s, double lam, double *delta)
{
    double A[6][6], b[6];
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int c = a; c < 6; c++) A[a][c] = s[e++];
#pragma unroll
    for (int a = 0; a < 6; a++) { A[a][a] = A[a][a] + lam * A[a][a]; b[a] = -s[21 + a]; }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double d = A[k][k];
        ok = ok && (d >= kPnpPivot);
#pragma unroll
        for (int i = k + 1; i < 6; i++) {
            const double l = A[k][i] / d;
#pragma unroll
            for (int j = i; j < 6; j++) A[i][j] = A[i][j] - l * A[k][j];
            b[i] = b[i] - l * b[k];
        }
    }
#pragma unroll
    for (int k = 5; k >= 0; k--) {
        double acc = b[k];
#pragma unroll
        for (int j = k + 1; j < 6; j++) acc = acc - A[k][j] * delta[j];
        delta[k] = acc / A[k][k];
    }
    return ok;
}

PNP_HD void pnp_update(PnpPose &P, const double *delta)
{
    P.t[0] = P.t[0] + delta[0]; P.t[1] = P.t[1] + delta[1]; P.t[2] = P.t[2] + delta[2];
    const double dq[4] = { delta[3] * 0.5, delta[4] * 0.5, delta[5] * 0.5, 1.0 };
    double q[4];
    pnp_qmul(P.q, dq, q);
    pnp_qnormalise(q);
    P.q[0] = q[0]; P.q[1] = q[1]; P.q[2] = q[2]; P.q[3] = q[3];
}
// lambda of step k: 4^-k while k < kPnpDamp, then 0
PNP_HD double pnp_lambda(int k)
{
    double lam = 1.0;
    for (int i = 0; i < k; i++) lam = lam * 0.25;
    return k < kPnpDamp ? lam : 0.0;
}

// The minimal solve: kPnpIters steps from P on the four sampled points; pd is [5][kPnpPts] (X, Y, Z, u, v).  false: invalid
PNP_HD bool pnp_solve4(const double *pd, const int *idx, PnpPose &P)
{
    for (int it = 0; it < kPnpIters; it++) {
        double R[9], s[kPnpC], c[kPnpC], delta[6];
        pnp_rot(P.q, R);
#pragma unroll
        for (int e = 0; e < kPnpC; e++) s[e] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = idx[k];
            const double X[3] = { pd[i], pd[kPnpPts + i], pd[2 * kPnpPts + i] };
            if (!pnp_contrib(R, P.t, X, pd[3 * kPnpPts + i], pd[4 * kPnpPts + i], c)) return false;
#pragma unroll
            for (int e = 0; e < kPnpC; e++) s[e] = s[e] + c[e];
        }
        if (!pnp_solve6(s, pnp_lambda(it), delta)) return false;
        pnp_update(P, delta);
    }
    // the pose must see its own sample in front of it, and be a number
    double R[9];
    pnp_rot(P.q, R);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = idx[k];
        const double X[3] = { pd[i], pd[kPnpPts + i], pd[2 * kPnpPts + i] };
        double p[3];
        pnp_apply(R, P.t, X, p);
        if (!(p[2] > 0.0)) return false;
    }
    return true;
}

PNP_HD int pnp_count(const double *pd, int m, const PnpPose &P, double thr2)
{
    double R[9];
    pnp_rot(P.q, R);
    int cnt = 0;
    for (int i = 0; i < m; i++) {
        const double X[3] = { pd[i], pd[kPnpPts + i], pd[2 * kPnpPts + i] };
        cnt += pnp_inlier(R, P.t, X, pd[3 * kPnpPts + i], pd[4 * kPnpPts + i], thr2) ? 1 : 0;
    }
    return cnt;
}

// larger key: more inliers, then the lower h; never 0 for a valid hypothesis
PNP_HD unsigned int pnp_pack(int inliers, int h) { return ((unsigned int)inliers << 16) | (0xFFFFu - (unsigned int)h); }

// nullptr: well-formed; otherwise what is wrong (feat_check.hpp style).  0 selects a parameter's default
static inline const char *pnp_check_params(double threshold, int n_hyp, int min_brief, int min_pnp, double angle, double trans)
{
    if (!(threshold >= 0.0) || std::isinf(threshold)) return "threshold must be a finite number >= 0 (0: 10 / 460)";
    if (n_hyp < 0 || n_hyp > kPnpMaxHyp) return "n_hyp must be 0..1024 (0: 256)";
    if (min_brief < 0 || min_pnp < 0) return "min_brief_loop_num and min_pnp_loop_num must not be negative (0: 25 and 5)";
    if (!(angle >= 0.0) || !(trans >= 0.0)) return "angle_threshold and trans_threshold must be >= 0 (0: 30 degrees and 20 m)";
    return nullptr;
}

// ---- after the pose: host code (atan2, sin, cos), fp64, compared with the restatement to a tolerance --------------------------------
// math_utils.h:187-202 (degrees) on a row-major R, and :252-260
inline void pnp_r2ypr(const double *R, double *ypr)
{
    const double y = atan2(R[3], R[0]);
    const double p = atan2(-R[6], R[0] * cos(y) + R[3] * sin(y));
    const double r = atan2(R[2] * sin(y) - R[5] * cos(y), -R[1] * sin(y) + R[4] * cos(y));
    ypr[0] = y / M_PI * 180.0; ypr[1] = p / M_PI * 180.0; ypr[2] = r / M_PI * 180.0;
}
inline double pnp_normalize_angle(double a)
{
    return a > 0 ? a - 360.0 * floor((a + 180.0) / 360.0) : a + 360.0 * floor((-a + 180.0) / 360.0);
}

struct PnpLoop { double t_old[3], q_old[4], rel_t[3], rel_q[4], rel_yaw, rel_euler[3]; bool within; };

// KeyFrame.cc:341-350 and :572-575, :588 from the camera-from-world pose of the old keyframe (host, fp64; compared to a tolerance)
inline void pnp_after(const double *pose_tq, const double *vio_tq, const double *ex_tq, double angle, double trans, PnpLoop &L)
{
    const double qwc[4] = { -pose_tq[3], -pose_tq[4], -pose_tq[5], pose_tq[6] }, qcl[4] = { -ex_tq[3], -ex_tq[4], -ex_tq[5], ex_tq[6] };
    const double zero[3] = { 0.0, 0.0, 0.0 }, mt[3] = { -pose_tq[0], -pose_tq[1], -pose_tq[2] };
    double Rwc[9], Ro[9], Rv[9], twc[3], rt[3];
    pnp_rot(qwc, Rwc);
    pnp_apply(Rwc, zero, mt, twc);                       // T_w_c_old = R_w_c_old (-T_pnp)
    pnp_qmul(qwc, qcl, L.q_old);                         // PnP_R_old = R_w_c_old qlc^T
    pnp_rot(L.q_old, Ro);
    pnp_apply(Ro, zero, ex_tq, rt);
    for (int e = 0; e < 3; e++) L.t_old[e] = twc[e] - rt[e];
    const double d[3] = { vio_tq[0] - L.t_old[0], vio_tq[1] - L.t_old[1], vio_tq[2] - L.t_old[2] };
    for (int e = 0; e < 3; e++) L.rel_t[e] = Ro[e] * d[0] + Ro[3 + e] * d[1] + Ro[6 + e] * d[2];
    const double qoc[4] = { -L.q_old[0], -L.q_old[1], -L.q_old[2], L.q_old[3] };
    pnp_qmul(qoc, vio_tq + 3, L.rel_q);
    pnp_rot(vio_tq + 3, Rv);
    double ev[3], eo[3];
    pnp_r2ypr(Rv, ev); pnp_r2ypr(Ro, eo);
    L.rel_yaw = pnp_normalize_angle(ev[0] - eo[0]);
    for (int e = 0; e < 3; e++) L.rel_euler[e] = ev[e] - eo[e];
    const double en = sqrt(L.rel_euler[0] * L.rel_euler[0] + L.rel_euler[1] * L.rel_euler[1] + L.rel_euler[2] * L.rel_euler[2]);
    const double tn = sqrt(L.rel_t[0] * L.rel_t[0] + L.rel_t[1] * L.rel_t[1] + L.rel_t[2] * L.rel_t[2]);
    L.within = fabs(en) < angle && tn < trans;
}

// the 15 values of :658-682 from the old keyframe's pose (T_w_i, R_w_i) and the current keyframe's index
inline void pnp_channel(const double *old_tq, const PnpLoop &L, int cur, double *d)
{
    double Ro[9], ct[3], cq[4];
    pnp_rot(old_tq + 3, Ro);
    pnp_apply(Ro, old_tq, L.rel_t, ct);
    pnp_qmul(old_tq + 3, L.rel_q, cq);
    d[0] = old_tq[0]; d[1] = old_tq[1]; d[2] = old_tq[2]; d[3] = old_tq[6]; d[4] = old_tq[3]; d[5] = old_tq[4]; d[6] = old_tq[5];
    d[7] = ct[0]; d[8] = ct[1]; d[9] = ct[2]; d[10] = cq[3]; d[11] = cq[0]; d[12] = cq[1]; d[13] = cq[2]; d[14] = (double)cur;
}
inline void pnp_loop_info(const PnpLoop &L, double *d)
{
    d[0] = L.rel_t[0]; d[1] = L.rel_t[1]; d[2] = L.rel_t[2]; d[3] = L.rel_q[3]; d[4] = L.rel_q[0]; d[5] = L.rel_q[1]; d[6] = L.rel_q[2]; d[7] = L.rel_yaw;
}

#if !defined(__HIPCC__)
// The whole step on the host, in the kernel's order (the refit's sums in the kernel's tree: thread t adds the points t and t + 256,
// a butterfly over the 64 lanes of each wave, then (w0 + w1) + (w2 + w3)).  m pairs p3 [m][3], p2 [m][2] (fp32), status [m], pose [7], stats [4]
inline void pnp_ransac_host(int m, const float *p3, const float *p2, const double *guess_tq, int n_hyp, uint32_t seed, uint32_t key, double thr2,
                            unsigned char *status, double *pose_tq, int *stats)
{
    static thread_local double pd[5 * kPnpPts], part[kPnpT][kPnpC], tmp[kPnpT][kPnpC];
    for (int i = 0; i < m; i++) status[i] = 0;
    for (int e = 0; e < 7; e++) pose_tq[e] = guess_tq[e];
    if (m < 4 || m > kPnpPts) { for (int e = 0; e < 4; e++) stats[e] = -1; return; }
    for (int i = 0; i < m; i++) {
        pd[i] = (double)p3[3 * i]; pd[kPnpPts + i] = (double)p3[3 * i + 1]; pd[2 * kPnpPts + i] = (double)p3[3 * i + 2];
        pd[3 * kPnpPts + i] = (double)p2[2 * i]; pd[4 * kPnpPts + i] = (double)p2[2 * i + 1];
    }
    PnpPose G, best_pose{};
    for (int e = 0; e < 3; e++) G.t[e] = guess_tq[e];
    for (int e = 0; e < 4; e++) G.q[e] = guess_tq[3 + e];
    unsigned int best = 0u;
    int nvalid = 0;
    for (int h = 0; h < n_hyp; h++) {
        int idx[4];
        PnpPose P = G;
        if (!pnp_sample(pnp_key(seed, key, (uint32_t)h), m, idx) || !pnp_solve4(pd, idx, P)) continue;
        nvalid++;
        const unsigned int k = pnp_pack(pnp_count(pd, m, P, thr2), h);
        if (k > best) { best = k; best_pose = P; }
    }
    const int bcnt = (int)(best >> 16), bh = best ? (int)(0xFFFFu - (best & 0xFFFFu)) : -1;
    stats[0] = nvalid; stats[1] = bh; stats[2] = bcnt; stats[3] = 0;
    if (best == 0u || bcnt < 4) return;
    PnpPose P = best_pose;
    {
        double R[9];
        pnp_rot(P.q, R);
        for (int i = 0; i < m; i++) {
            const double X[3] = { pd[i], pd[kPnpPts + i], pd[2 * kPnpPts + i] };
            status[i] = pnp_inlier(R, P.t, X, pd[3 * kPnpPts + i], pd[4 * kPnpPts + i], thr2) ? 1 : 0;
        }
    }
    int done = 0;
    for (int it = 0; it < kPnpIters; it++) {
        double R[9], c[kPnpC], s[kPnpC], delta[6];
        pnp_rot(P.q, R);
        bool behind = false;
        for (int t = 0; t < kPnpT; t++) {
            for (int e = 0; e < kPnpC; e++) part[t][e] = 0.0;
            for (int i = t; i < m; i += kPnpT) {
                if (!status[i]) continue;
                const double X[3] = { pd[i], pd[kPnpPts + i], pd[2 * kPnpPts + i] };
                if (!pnp_contrib(R, P.t, X, pd[3 * kPnpPts + i], pd[4 * kPnpPts + i], c)) { behind = true; continue; }
                for (int e = 0; e < kPnpC; e++) part[t][e] = part[t][e] + c[e];
            }
        }
        if (behind) break;
        for (int o = 32; o > 0; o >>= 1) {
            for (int t = 0; t < kPnpT; t++) for (int e = 0; e < kPnpC; e++) tmp[t][e] = part[t][e] + part[t ^ o][e];
            for (int t = 0; t < kPnpT; t++) for (int e = 0; e < kPnpC; e++) part[t][e] = tmp[t][e];
        }
        for (int e = 0; e < kPnpC; e++) s[e] = (part[0][e] + part[64][e]) + (part[128][e] + part[192][e]);
        if (!pnp_solve6(s, pnp_lambda(it), delta)) break;
        pnp_update(P, delta);
        done++;
    }
    stats[3] = done;
    for (int e = 0; e < 3; e++) pose_tq[e] = P.t[e];
    for (int e = 0; e < 4; e++) pose_tq[3 + e] = P.q[e];
}
#endif

#if defined(__HIPCC__)

struct PnpJob {
    const float *p3, *p2;              // [n_src][3], [n_src][2]
    const unsigned char *sel;          // [n_src] (1: the pair takes part) or null: all do
    const int *count;                  // null, or the candidate's match count: at or below `gate` the step does not run
    int n_src, gate, n_hyp;
    unsigned int seed, key;
    double thr2;
    double guess[7];
    unsigned char *status;             // [n_src]
    double *pose;                      // [7]
    int *stats;                        // [4]
};

// One workgroup per candidate.  The selected pairs are compacted in order into LDS; thread t solves and scores the hypotheses t, t + 256, ...
__global__ __launch_bounds__(kPnpT) void k_pnp_ransac(const PnpJob *jobs)
{
    __shared__ double s_pd[5 * kPnpPts], s_part[2][4][kPnpC], s_pose[7];
    __shared__ unsigned int s_best;
    __shared__ int s_m, s_nvalid, s_bad;
    __shared__ unsigned short s_idx[kPnpPts];
    __shared__ unsigned char s_flag[kPnpPts], s_in[kPnpPts];
    const PnpJob &j = jobs[blockIdx.x];
    const int tid = threadIdx.x, n = min(max(j.n_src, 0), kPnpPts);
    for (int i = tid; i < kPnpPts; i += kPnpT) { s_flag[i] = (i < n && (!j.sel || j.sel[i])) ? 1 : 0; s_in[i] = 0; }
    if (tid == 0) { s_best = 0u; s_nvalid = 0; }
    __syncthreads();
    {
        const int i0 = tid, i1 = tid + kPnpT;
        int r0 = 0, r1 = 0, tot = 0;
        for (int k = 0; k < n; k++) { const int f = s_flag[k]; tot += f; r0 += k < i0 ? f : 0; r1 += k < i1 ? f : 0; }
        if (i0 < n && s_flag[i0]) s_idx[r0] = (unsigned short)i0;
        if (i1 < n && s_flag[i1]) s_idx[r1] = (unsigned short)i1;
        if (tid == 0) s_m = tot;
    }
    __syncthreads();
    const int m = s_m;
    const bool gated = j.count && *j.count <= j.gate;
    if (m < 4 || gated) {       // the step does not run
        for (int i = tid; i < n; i += kPnpT) j.status[i] = 0;
        if (tid < 4) j.stats[tid] = -1;
        if (tid < 7) j.pose[tid] = j.guess[tid];
        return;
    }
    for (int k = tid; k < m; k += kPnpT) {
        const int slot = s_idx[k];
        s_pd[k] = (double)j.p3[3 * slot]; s_pd[kPnpPts + k] = (double)j.p3[3 * slot + 1]; s_pd[2 * kPnpPts + k] = (double)j.p3[3 * slot + 2];
        s_pd[3 * kPnpPts + k] = (double)j.p2[2 * slot]; s_pd[4 * kPnpPts + k] = (double)j.p2[2 * slot + 1];
    }
    __syncthreads();
    PnpPose G;
#pragma unroll
    for (int e = 0; e < 3; e++) G.t[e] = j.guess[e];
#pragma unroll
    for (int e = 0; e < 4; e++) G.q[e] = j.guess[3 + e];
    const int nh = min(max(j.n_hyp, 0), kPnpMaxHyp);
    const double thr2 = j.thr2;
    unsigned int best = 0u;
    int nvalid = 0;
    PnpPose Pb = G;
    for (int h = tid; h < nh; h += kPnpT) {
        int idx[4];
        PnpPose P = G;
        if (!pnp_sample(pnp_key(j.seed, j.key, (uint32_t)h), m, idx) || !pnp_solve4(s_pd, idx, P)) continue;
        nvalid++;
        const unsigned int k = pnp_pack(pnp_count(s_pd, m, P, thr2), h);
        if (k > best) { best = k; Pb = P; }
    }
    if (best) atomicMax(&s_best, best);
    if (nvalid) atomicAdd(&s_nvalid, nvalid);
    __syncthreads();
    const unsigned int bk = s_best;
    const int bcnt = (int)(bk >> 16), bh = bk ? (int)(0xFFFFu - (bk & 0xFFFFu)) : -1;
    if (bk == 0u || bcnt < 4) {         // solvePnPRansac returning false: an empty inlier list, the guess unchanged
        for (int i = tid; i < n; i += kPnpT) j.status[i] = 0;
        if (tid == 0) { j.stats[0] = s_nvalid; j.stats[1] = bh; j.stats[2] = bcnt; j.stats[3] = 0; }
        if (tid < 7) j.pose[tid] = j.guess[tid];
        return;
    }
    if (best == bk) {                   // one thread: every key holds its own h
#pragma unroll
        for (int e = 0; e < 3; e++) s_pose[e] = Pb.t[e];
#pragma unroll
        for (int e = 0; e < 4; e++) s_pose[3 + e] = Pb.q[e];
    }
    __syncthreads();
    PnpPose P;
#pragma unroll
    for (int e = 0; e < 3; e++) P.t[e] = s_pose[e];
#pragma unroll
    for (int e = 0; e < 4; e++) P.q[e] = s_pose[3 + e];
    {
        double R[9];
        pnp_rot(P.q, R);
        for (int k = tid; k < m; k += kPnpT) {
            const double X[3] = { s_pd[k], s_pd[kPnpPts + k], s_pd[2 * kPnpPts + k] };
            s_in[k] = pnp_inlier(R, P.t, X, s_pd[3 * kPnpPts + k], s_pd[4 * kPnpPts + k], thr2) ? 1 : 0;
        }
    }
    __syncthreads();
    // refit over the winner's inliers: every thread carries the pose and takes the same step
    int done = 0;
    for (int it = 0; it < kPnpIters; it++) {
        double R[9], c[kPnpC], s[kPnpC], delta[6];
        pnp_rot(P.q, R);
        if (tid == 0) s_bad = 0;
#pragma unroll
        for (int e = 0; e < kPnpC; e++) s[e] = 0.0;
        bool behind = false;
        for (int k = tid; k < m; k += kPnpT) {
            if (!s_in[k]) continue;
            const double X[3] = { s_pd[k], s_pd[kPnpPts + k], s_pd[2 * kPnpPts + k] };
            if (!pnp_contrib(R, P.t, X, s_pd[3 * kPnpPts + k], s_pd[4 * kPnpPts + k], c)) { behind = true; continue; }
#pragma unroll
            for (int e = 0; e < kPnpC; e++) s[e] = s[e] + c[e];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int e = 0; e < kPnpC; e++) s[e] = s[e] + __shfl_xor(s[e], o);
        __syncthreads();                // s_bad is reset, the other buffer of s_part is free
        if (behind) atomicOr(&s_bad, 1);
        if ((tid & (kWave - 1)) == 0)
#pragma unroll
            for (int e = 0; e < kPnpC; e++) s_part[it & 1][tid / kWave][e] = s[e];
        __syncthreads();
        if (s_bad) break;
#pragma unroll
        for (int e = 0; e < kPnpC; e++) s[e] = (s_part[it & 1][0][e] + s_part[it & 1][1][e]) + (s_part[it & 1][2][e] + s_part[it & 1][3][e]);
        if (!pnp_solve6(s, pnp_lambda(it), delta)) break;        // uniform: every thread holds the same sums
        pnp_update(P, delta);
        done++;
    }
    for (int i = tid; i < kPnpPts; i += kPnpT) s_flag[i] = 0;
    __syncthreads();
    for (int k = tid; k < m; k += kPnpT) if (s_in[k]) s_flag[s_idx[k]] = 1;
    __syncthreads();
    for (int i = tid; i < n; i += kPnpT) j.status[i] = s_flag[i];
    if (tid == 0) {
        j.stats[0] = s_nvalid; j.stats[1] = bh; j.stats[2] = bcnt; j.stats[3] = done;
#pragma unroll
        for (int e = 0; e < 3; e++) j.pose[e] = P.t[e];
#pragma unroll
        for (int e = 0; e < 4; e++) j.pose[3 + e] = P.q[e];
    }
}

#endif // __HIPCC__

} // namespace lmono
