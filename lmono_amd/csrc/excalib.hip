// excalib.hip -- the camera-LiDAR rotation calibration of ESTIMATE_LASER == 2 (Estimator.cc:403-430, src/initial/AxxbSolver.cc) on the
// device: DESIGN.md 6i.  Four stages per stream and frame: (1) the essential matrix of the frame's point pairs, the Hartley-normalised
// 8-point fit over all of them (what cv::findFundamentalMat's RANSAC returns at a threshold of 3.0 on normalised points: every pair is an
// inlier); (2) its decomposition into R1, R2, +-t; (3) the cheirality vote of testTriangulation over the four combinations; (4) one step
// of CalibrationExRotation on a running 4 x 4 sum.  Every step is one IEEE fp64 operation in the order written here and in
// tests/excalib_ref.py (the library is built with -ffp-contract=off).  The arithmetic (exc_*) is plain C++ and also compiles for the
// host (lmono_amd/host/excalib_test.cpp); rej_jacobi, rej_smallest, rej_refit and rej_denorm are the tracker's (track_reject.hip).
#pragma once
#if defined(__HIPCC__)
#include "track.hip"
#else
#include "track_reject.hip"
#endif

namespace lmono {

constexpr int kExcT = 256;            // threads of the workgroup
constexpr int kExcMinPairs = 9;       // AxxbSolver.cc:16
constexpr int kExcSweeps3 = 6;        // cyclic Jacobi sweeps of the 3 x 3 and 4 x 4 problems (the measured residues)
constexpr int kExcSweeps4 = 7;
constexpr double kExcDeg = 57.295779513082323;   // 180 / pi
constexpr int kExcRel = 1, kExcCal = 2;           // ExcJob::mode bits: stages 1-3, stage 4

// the calibration state of one stream: A^T A of CalibrationExRotation's 4k x 4 matrix, rlc, frame_count
struct ExcState { double M[16]; double rlc[9]; int frame_count; int pad; };

REJ_HD bool exc_finite(double v) { return v - v == 0.0; }

REJ_HD void exc_identity(double *R)
{
    for (int e = 0; e < 9; e++) R[e] = (e % 4 == 0) ? 1.0 : 0.0;
}

// ---- stage 1: the sums of the normalisation and of the 9 x 9 normal matrix.  pd: [4][kRejPts] (prev x, prev y, cur x, cur y), m pairs.
// Each sum runs over ascending pair index, so its tree depends on m alone.
REJ_HD double exc_mean(const double *pd, int m, int col)
{
    double acc = 0.0;
    for (int k = 0; k < m; k++) acc = acc + pd[col * kRejPts + k];
    return acc / (double)m;
}
// mean distance from (mx, my) of image `img` (0: prev, 1: cur)
REJ_HD double exc_dist(const double *pd, int m, int img, double mx, double my)
{
    double acc = 0.0;
    for (int k = 0; k < m; k++) {
        const double ax = pd[2 * img * kRejPts + k] - mx, ay = pd[(2 * img + 1) * kRejPts + k] - my;
        acc = acc + sqrt(ax * ax + ay * ay);
    }
    return acc / (double)m;
}
// entry e (0..44) of the upper triangle of M = A^T A -> (a, b), a <= b
REJ_HD void exc_pair_of(int e, int &a, int &b)
{
    a = 0;
    while (e >= 9 - a) { e -= 9 - a; a++; }
    b = a + e;
}
REJ_HD double exc_normal_entry(const double *pd, int m, int a, int b, double sp, double mpx, double mpy, double sc, double mcx, double mcy)
{
    double acc = 0.0;
    for (int k = 0; k < m; k++) {
        const double l0 = (pd[k] - mpx) * sp, l1 = (pd[kRejPts + k] - mpy) * sp;
        const double r0 = (pd[2 * kRejPts + k] - mcx) * sc, r1 = (pd[3 * kRejPts + k] - mcy) * sc;
        acc = acc + (rej_pick(a / 3, l0, l1) * rej_pick(a % 3, r0, r1)) * (rej_pick(b / 3, l0, l1) * rej_pick(b % 3, r0, r1));
    }
    return acc;
}

// rej_refit's F has prev^T F cur = 0; cv::findFundamentalMat(prev, cur) has cur^T E prev = 0: its transpose
REJ_HD void exc_transpose3(double *E)
{
    double s;
    s = E[1]; E[1] = E[3]; E[3] = s;
    s = E[2]; E[2] = E[6]; E[6] = s;
    s = E[5]; E[5] = E[7]; E[7] = s;
}

// ---- stage 2: E -> R1 = U W V^T, R2 = U W^T V^T (R12 [18]), t = u3 (the other translation is -t).  V from Jacobi on E^T E, the two
// larger eigenvalues first (the larger of them first, the lower index on a tie); u_i = E v_i / |E v_i|, u3 = u1 x u2, v3 = v1 x v2.
// U and V are proper by construction, so det R1 = det R2 = +1 and the reference's -E branch (AxxbSolver.cc:28-32) cannot fire.
REJ_HD void exc_decompose(const double *E, double *R12, double *t)
{
    double G[9], V[9];
    for (int a = 0; a < 3; a++)
        for (int c = a; c < 3; c++) {
            const double g = (E[a] * E[c] + E[3 + a] * E[3 + c]) + E[6 + a] * E[6 + c];
            G[a * 3 + c] = g; G[c * 3 + a] = g;
        }
    rej_jacobi<3>(G, V, kExcSweeps3);
    const int b = rej_smallest<3>(G);
    int i1 = (b == 0) ? 1 : 0, i2 = (b == 2) ? 1 : 2;
    if (G[i2 * 3 + i2] > G[i1 * 3 + i1]) { const int s = i1; i1 = i2; i2 = s; }
    double v[3][3], u[3][3];
    for (int r = 0; r < 3; r++) { v[0][r] = V[r * 3 + i1]; v[1][r] = V[r * 3 + i2]; }
    for (int i = 0; i < 2; i++) {
        const double a0 = (E[0] * v[i][0] + E[1] * v[i][1]) + E[2] * v[i][2];
        const double a1 = (E[3] * v[i][0] + E[4] * v[i][1]) + E[5] * v[i][2];
        const double a2 = (E[6] * v[i][0] + E[7] * v[i][1]) + E[8] * v[i][2];
        const double nrm = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
        u[i][0] = a0 / nrm; u[i][1] = a1 / nrm; u[i][2] = a2 / nrm;
    }
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1]; u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2]; u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    v[2][0] = v[0][1] * v[1][2] - v[0][2] * v[1][1]; v[2][1] = v[0][2] * v[1][0] - v[0][0] * v[1][2]; v[2][2] = v[0][0] * v[1][1] - v[0][1] * v[1][0];
    for (int i = 0; i < 3; i++)
        for (int jj = 0; jj < 3; jj++) {
            R12[3 * i + jj] = (u[1][i] * v[0][jj] - u[0][i] * v[1][jj]) + u[2][i] * v[2][jj];
            R12[9 + 3 * i + jj] = (u[0][i] * v[1][jj] - u[1][i] * v[0][jj]) + u[2][i] * v[2][jj];
        }
    t[0] = u[2][0]; t[1] = u[2][1]; t[2] = u[2][2];
}

// ---- stage 3: is the DLT point of one pair in front of P = [I | 0] and P1 = [R | t] (testTriangulation, AxxbSolver.cc:46-70)?
// The rows are cv::triangulatePoints': x P[2] - P[0], y P[2] - P[1] per camera; X = the smallest eigenvector of A^T A.
REJ_HD bool exc_front(const double *R, const double *t, double px, double py, double cx, double cy)
{
    double A[16], B[16], V[16];
    A[0] = -1.0; A[1] = 0.0; A[2] = px; A[3] = 0.0;
    A[4] = 0.0; A[5] = -1.0; A[6] = py; A[7] = 0.0;
    for (int c = 0; c < 3; c++) { A[8 + c] = cx * R[6 + c] - R[c]; A[12 + c] = cy * R[6 + c] - R[3 + c]; }
    A[11] = cx * t[2] - t[0]; A[15] = cy * t[2] - t[1];
    for (int a = 0; a < 4; a++)
        for (int c = a; c < 4; c++) {
            const double g = ((A[a] * A[c] + A[4 + a] * A[4 + c]) + A[8 + a] * A[8 + c]) + A[12 + a] * A[12 + c];
            B[a * 4 + c] = g; B[c * 4 + a] = g;
        }
    rej_jacobi<4>(B, V, kExcSweeps4);
    const int b = rej_smallest<4>(B);
    const double w = V[12 + b];
    if (w == 0.0 || !exc_finite(w)) return false;
    const double X = V[b] / w, Y = V[4 + b] / w, Z = V[8 + b] / w;
    const double zr = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2];
    return Z > 0.0 && zr > 0.0;
}

// the vote over the four front counts (R1 t, R1 -t, R2 t, R2 -t): R1 on a strict majority, else R2; the winner transposed, or the
// identity (winner -1) when an entry of it is not finite
REJ_HD int exc_vote(const double *R12, const int *cnt, double *R_out)
{
    const int c1 = cnt[0] > cnt[1] ? cnt[0] : cnt[1], c2 = cnt[2] > cnt[3] ? cnt[2] : cnt[3];
    const int win = c1 > c2 ? 0 : 1;
    bool fin = true;
    for (int e = 0; e < 9; e++) fin = fin && exc_finite(R12[9 * win + e]);
    if (!fin) { exc_identity(R_out); return -1; }
    for (int i = 0; i < 3; i++) for (int jj = 0; jj < 3; jj++) R_out[3 * jj + i] = R12[9 * win + 3 * i + jj];
    return win;
}

// ---- stage 4 -------------------------------------------------------------------------------------------------------------------------
// Eigen's Quaterniond::toRotationMatrix; q = (x, y, z, w), not normalised
REJ_HD void exc_q2m(const double *q, double *R)
{
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}
// Eigen's Quaterniond(Matrix3d): the trace branch and the three diagonal branches
REJ_HD void exc_m2q(const double *R, double *q)
{
    double tr = (R[0] + R[4]) + R[8];
    if (tr > 0.0) {
        tr = sqrt(tr + 1.0);
        q[3] = 0.5 * tr;
        tr = 0.5 / tr;
        q[0] = (R[7] - R[5]) * tr; q[1] = (R[2] - R[6]) * tr; q[2] = (R[3] - R[1]) * tr;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int jj = (i + 1) % 3, k = (jj + 1) % 3;
        double s = sqrt(((R[4 * i] - R[4 * jj]) - R[4 * k]) + 1.0);
        q[i] = 0.5 * s;
        s = 0.5 / s;
        q[3] = (R[3 * k + jj] - R[3 * jj + k]) * s;
        q[jj] = (R[3 * jj + i] + R[3 * i + jj]) * s;
        q[k] = (R[3 * k + i] + R[3 * i + k]) * s;
    }
}
REJ_HD void exc_mul33(const double *A, const double *B, double *C)
{
    for (int i = 0; i < 3; i++)
        for (int jj = 0; jj < 3; jj++) C[3 * i + jj] = (A[3 * i] * B[jj] + A[3 * i + 1] * B[3 + jj]) + A[3 * i + 2] * B[6 + jj];
}
// Quaterniond::angularDistance in degrees: 2 atan2(|vec|, |w|) of a b*
REJ_HD double exc_angle_deg(const double *a, const double *b)
{
    const double cx = -b[0], cy = -b[1], cz = -b[2], cw = b[3];
    const double w = ((a[3] * cw - a[0] * cx) - a[1] * cy) - a[2] * cz;
    const double x = ((a[3] * cx + a[0] * cw) + a[1] * cz) - a[2] * cy;
    const double y = ((a[3] * cy + a[1] * cw) + a[2] * cx) - a[0] * cz;
    const double z = ((a[3] * cz + a[2] * cw) + a[0] * cy) - a[1] * cx;
    const double nv = sqrt((x * x + y * y) + z * z);
    return kExcDeg * (2.0 * atan2(nv, fabs(w)));
}
// One step of CalibrationExRotation (AxxbSolver.cc:89-147) on the running sum.  st is read and written; rlc_out [9], sv [4] descending,
// *huber the weight of this frame's block; -> ok.
REJ_HD bool exc_calib(ExcState &st, const double *q_cam, const double *q_lidar, int count, double *rlc_out, double *sv, double *huber)
{
    st.frame_count = st.frame_count + 1;
    double Rc[9], Rl[9], Rt[9], T[9], Rg[9], r1[4], r2[4], rl[4];
    exc_q2m(q_cam, Rc);
    exc_q2m(q_lidar, Rl);
    for (int i = 0; i < 3; i++) for (int jj = 0; jj < 3; jj++) Rt[3 * i + jj] = st.rlc[3 * jj + i];
    exc_mul33(Rt, Rl, T);
    exc_mul33(T, st.rlc, Rg);
    exc_m2q(Rc, r1); exc_m2q(Rg, r2); exc_m2q(Rl, rl);
    const double deg = exc_angle_deg(r1, r2);
    const double hub = deg > 5.0 ? 5.0 / deg : 1.0;
    *huber = hub;
    // L(r1) - R(rl), row-major
    double D[16];
    {
        const double x = r1[0], y = r1[1], z = r1[2], w = r1[3], a = rl[0], b = rl[1], c = rl[2], d = rl[3];
        D[0] = w - d; D[1] = -z - c; D[2] = y - (-b); D[3] = x - a;
        D[4] = z - (-c); D[5] = w - d; D[6] = -x - a; D[7] = y - b;
        D[8] = -y - b; D[9] = x - (-a); D[10] = w - d; D[11] = z - c;
        D[12] = -x - (-a); D[13] = -y - (-b); D[14] = -z - (-c); D[15] = w - d;
    }
    for (int e = 0; e < 16; e++) D[e] = hub * D[e];
    for (int a = 0; a < 4; a++)
        for (int c = a; c < 4; c++) {
            const double g = ((D[a] * D[c] + D[4 + a] * D[4 + c]) + D[8 + a] * D[8 + c]) + D[12 + a] * D[12 + c];
            const double s = st.M[a * 4 + c] + g;
            st.M[a * 4 + c] = s; st.M[c * 4 + a] = s;
        }
    double W[16], V[16];
    for (int e = 0; e < 16; e++) W[e] = st.M[e];
    rej_jacobi<4>(W, V, kExcSweeps4);
    const int b = rej_smallest<4>(W);
    const double x[4] = { V[b], V[4 + b], V[8 + b], V[12 + b] };
    double Rx[9];
    exc_q2m(x, Rx);
    for (int i = 0; i < 3; i++) for (int jj = 0; jj < 3; jj++) st.rlc[3 * i + jj] = Rx[3 * jj + i];
    for (int e = 0; e < 9; e++) rlc_out[e] = st.rlc[e];
    for (int i = 0; i < 4; i++) { const double l = W[5 * i]; sv[i] = sqrt(l > 0.0 ? l : 0.0); }
    for (int i = 1; i < 4; i++)             // insertion sort, descending
        for (int k = i; k > 0 && sv[k] > sv[k - 1]; k--) { const double s = sv[k]; sv[k] = sv[k - 1]; sv[k - 1] = s; }
    return st.frame_count >= count && sv[2] > 0.25;
}

// ---- the whole step on the host, in the kernel's order (excalib_test; pairs [m][4], any m) ---------------------------------------------
// stages 1-3: -> R_out [9], stats [6] = pairs used, the four front counts, the winner (0: R1, 1: R2, -1: the identity by rule)
inline void exc_relative_host(int m_in, const double *pairs, double *R_out, int *stats)
{
    static thread_local double pd[4 * kRejPts];
    int m = 0;
    for (int k = 0; k < m_in && k < kRejPts; k++) {
        const double *p = pairs + 4 * (size_t)k;
        if (!(exc_finite(p[0]) && exc_finite(p[1]) && exc_finite(p[2]) && exc_finite(p[3]))) continue;
        for (int c = 0; c < 4; c++) pd[c * kRejPts + m] = p[c];
        m++;
    }
    exc_identity(R_out);
    stats[0] = m; stats[1] = stats[2] = stats[3] = stats[4] = 0; stats[5] = -1;
    if (m < kExcMinPairs) return;
    const double mpx = exc_mean(pd, m, 0), mpy = exc_mean(pd, m, 1), mcx = exc_mean(pd, m, 2), mcy = exc_mean(pd, m, 3);
    const double dp = exc_dist(pd, m, 0, mpx, mpy), dc = exc_dist(pd, m, 1, mcx, mcy);
    if (!(dp > 0.0) || !(dc > 0.0)) return;
    const double sp = kRejSqrt2 / dp, sc = kRejSqrt2 / dc;
    double M[81], V[81], G[9], V3[9], E[9], R12[18], t[3], tn[3];
    for (int e = 0; e < 45; e++) {
        int a, b;
        exc_pair_of(e, a, b);
        const double v = exc_normal_entry(pd, m, a, b, sp, mpx, mpy, sc, mcx, mcy);
        M[a * 9 + b] = v; M[b * 9 + a] = v;
    }
    rej_refit(M, V, G, V3, sp, mpx, mpy, sc, mcx, mcy, E);
    exc_transpose3(E);
    exc_decompose(E, R12, t);
    for (int e = 0; e < 3; e++) tn[e] = -t[e];
    int cnt[4] = { 0, 0, 0, 0 };
    for (int combo = 0; combo < 4; combo++)
        for (int k = 0; k < m; k++)
            cnt[combo] += exc_front(R12 + 9 * (combo >> 1), (combo & 1) ? tn : t, pd[k], pd[kRejPts + k], pd[2 * kRejPts + k], pd[3 * kRejPts + k]) ? 1 : 0;
    for (int e = 0; e < 4; e++) stats[1 + e] = cnt[e];
    stats[5] = exc_vote(R12, cnt, R_out);
}

#if defined(__HIPCC__)

struct ExcJob {
    const double *pairs;        // [m][4]
    int m, mode, count, pad;
    double q_cam[4], q_lidar[4];    // q_cam: stage 4 alone (with stages 1-3 it is Quaterniond(R_cam))
    ExcState *state;
    double *R_cam;              // [9]
    int *stats;                 // [6]
    double *rlc, *sv, *huber;   // [9], [4], [1]
    int *ok;
};

// One workgroup per stream; a stream with nothing to do leaves at once.  m was validated on the host (0..kRejPts) and is clamped again:
// every LDS array is sized by the constant and no loop bound is read from device memory other than the job's own m.
__global__ __launch_bounds__(kExcT) void k_excalib_step(const ExcJob *jobs)
{
    __shared__ double s_pd[4 * kRejPts], s_M[81], s_V[81], s_G[9], s_V3[9], s_E[9], s_R12[18], s_t[6], s_nrm[6], s_Rcam[9];
    __shared__ unsigned short s_idx[kRejPts];
    __shared__ unsigned char s_flag[kRejPts];
    __shared__ int s_m, s_cnt[4];
    const ExcJob &j = jobs[blockIdx.x];
    const int mode = j.mode;
    if (!(mode & (kExcRel | kExcCal))) return;
    const int tid = threadIdx.x;
    if (mode & kExcRel) {
        const int n = min(max(j.m, 0), kRejPts);
        for (int i = tid; i < kRejPts; i += kExcT) {
            bool f = false;
            if (i < n) {
                const double *p = j.pairs + 4 * (size_t)i;
                f = exc_finite(p[0]) && exc_finite(p[1]) && exc_finite(p[2]) && exc_finite(p[3]);
            }
            s_flag[i] = f ? 1 : 0;
        }
        if (tid < 4) s_cnt[tid] = 0;
        __syncthreads();
        {   // the finite pairs in order
            const int i0 = tid, i1 = tid + kExcT;
            int r0 = 0, r1 = 0, tot = 0;
            for (int k = 0; k < n; k++) { const int f = s_flag[k]; tot += f; r0 += k < i0 ? f : 0; r1 += k < i1 ? f : 0; }
            if (i0 < n && s_flag[i0]) s_idx[r0] = (unsigned short)i0;
            if (i1 < n && s_flag[i1]) s_idx[r1] = (unsigned short)i1;
            if (tid == 0) s_m = tot;
        }
        __syncthreads();
        const int m = s_m;
        for (int k = tid; k < m; k += kExcT) {
            const double *p = j.pairs + 4 * (size_t)s_idx[k];
            s_pd[k] = p[0]; s_pd[kRejPts + k] = p[1]; s_pd[2 * kRejPts + k] = p[2]; s_pd[3 * kRejPts + k] = p[3];
        }
        __syncthreads();
        bool solved = m >= kExcMinPairs;
        if (solved) {
            if (tid < 4) s_nrm[tid] = exc_mean(s_pd, m, tid);
            __syncthreads();
            if (tid < 2) s_nrm[4 + tid] = exc_dist(s_pd, m, tid, s_nrm[2 * tid], s_nrm[2 * tid + 1]);
            __syncthreads();
            const double mpx = s_nrm[0], mpy = s_nrm[1], mcx = s_nrm[2], mcy = s_nrm[3], dp = s_nrm[4], dc = s_nrm[5];
            solved = dp > 0.0 && dc > 0.0;
            if (solved) {
                const double sp = kRejSqrt2 / dp, sc = kRejSqrt2 / dc;
                if (tid < 45) {
                    int a, b;
                    exc_pair_of(tid, a, b);
                    const double v = exc_normal_entry(s_pd, m, a, b, sp, mpx, mpy, sc, mcx, mcy);
                    s_M[a * 9 + b] = v; s_M[b * 9 + a] = v;
                }
                __syncthreads();
                if (tid == 0) {
                    rej_refit(s_M, s_V, s_G, s_V3, sp, mpx, mpy, sc, mcx, mcy, s_E);
                    exc_transpose3(s_E);
                    exc_decompose(s_E, s_R12, s_t);
                    for (int e = 0; e < 3; e++) s_t[3 + e] = -s_t[e];
                }
                __syncthreads();
                // the vote: one task per (combination, pair); integer counts, so their order does not matter
                int c[4] = { 0, 0, 0, 0 };
                for (int task = tid; task < 4 * m; task += kExcT) {
                    const int combo = task / m, k = task - combo * m;
                    const bool f = exc_front(s_R12 + 9 * (combo >> 1), s_t + 3 * (combo & 1), s_pd[k], s_pd[kRejPts + k], s_pd[2 * kRejPts + k], s_pd[3 * kRejPts + k]);
#pragma unroll
                    for (int e = 0; e < 4; e++) c[e] += (f && combo == e) ? 1 : 0;
                }
#pragma unroll
                for (int e = 0; e < 4; e++) if (c[e]) atomicAdd(&s_cnt[e], c[e]);
                __syncthreads();
            }
        }
        if (tid == 0) {
            int win = -1;
            if (solved) win = exc_vote(s_R12, s_cnt, s_Rcam); else exc_identity(s_Rcam);
            for (int e = 0; e < 9; e++) j.R_cam[e] = s_Rcam[e];
            j.stats[0] = m;
            for (int e = 0; e < 4; e++) j.stats[1 + e] = s_cnt[e];
            j.stats[5] = win;
        }
    }
    if ((mode & kExcCal) && tid == 0) {     // s_Rcam was written by this thread
        double qc[4], ql[4], rlc[9], sv[4], hub;
        if (mode & kExcRel) exc_m2q(s_Rcam, qc); else for (int e = 0; e < 4; e++) qc[e] = j.q_cam[e];
        for (int e = 0; e < 4; e++) ql[e] = j.q_lidar[e];
        ExcState st = *j.state;
        const bool ok = exc_calib(st, qc, ql, j.count, rlc, sv, &hub);
        *j.state = st;
        for (int e = 0; e < 9; e++) j.rlc[e] = rlc[e];
        for (int e = 0; e < 4; e++) j.sv[e] = sv[e];
        *j.huber = hub;
        *j.ok = ok ? 1 : 0;
    }
}

#endif // __HIPCC__

} // namespace lmono
