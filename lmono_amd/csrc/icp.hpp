// icp.hpp -- the arithmetic of the point-to-point ICP between the outlier filter and the voxel map: the pcl::IterativeClosestPoint
// that MapBuilder::processMapping carries commented out (mono_lidar_mapping/src/map_builder/Map_Builder.cc:31-59; setMaxCorrespondenceDistance(0.5),
// setMaximumIterations(50), setTransformationEpsilon(1e-8), setEuclideanFitnessEpsilon(1)).  One text for the kernels (icp.hip), for a CPU
// program (host/icp_test.cpp) and for the host side of the C ABI; every float operation is a single IEEE operation (build with
// -ffp-contract=off).  The definition is this project's own: the result is a pure function of the SET of target points and of the source
// points.  Parity with PCL is unpinned.
//
// Target.  A point is valid iff sor_cell accepts it at inv = 1.0f / h.  The origin o[a] = (min_a + max_a) * 0.5f over the valid points, min and max in
// the order of icp_ord (the float order, with -0 below +0, so that o has one definition).  w = m - o; a valid point with some |w_a| >= 2048 is out of
// span: counted as rejected, never a neighbour (these rules are the grid's: cell_grid.hpp).  iw_a = (int64)((double)w_a * 65536.0).
// Source.  p0 = (float)(G p) (icp_guess_axis: fp64, fixed order), u = p0 - o; usable iff every u_a is finite and |u_a| < 2048; iu as iw.
// State.  R (fp64, row-major) and tau (fp64) in origin-centred coordinates: x' - o = R (x - o) + tau.  They start at I and 0.
// Iteration k.  q = (float)((double)o + (R (double)u + tau)) (icp_q_axis).  q must be valid by sor_cell, else the point is unmatched.  Its
// correspondence is the target point with the smallest sor_d2(q, m); ties go to the smaller x, then y, then z (icp_better).  The pair is accepted
// iff d2 <= D * D (float32).  The sums over the accepted pairs are exact integers (IcpSums), so any reduction order gives the same words; the solve
// (icp_solve) is Horn's closed form with the 4 x 4 eigenproblem by rej_jacobi<4>, kIcpSweeps sweeps, and the stopping rule of icp_iterate:
//   status 0  both sum((tau' - tau)^2) < eps and sum((R' - R)^2) < eps
//   status 2  mse_eps > 0, k >= 2 and |mse_k - mse_(k-1)| < mse_eps, mse = (double)E / N / 2^24.  With the reference's mse_eps = 1 (m^2, against
//             squared distances of at most max_corr^2 = 0.25) this holds at the second iteration of every run that reaches it.
//   status 1  k == max_iter
//   status 3  fewer than 3 accepted pairs: the state is kept
// Result.  t = ((double)o + tau) - R o, composed with G in fp64 (icp_transform); always composed, so that the bytes have one definition.
//
// Why the grid cannot change the result: the argument at the head of sor.hpp for k = 1.  A search that has looked at every cell within ring r >= 1 of
// q's cell may stop as soon as its best d2 <= sor_rho2(r, h): every point of an unvisited cell has d2 > sor_rho2(r, h), so it is neither nearer nor
// a tie.  At r = max_rings, sor_rho(max_rings, h) >= D gives sor_rho2 >= D * D (float32 rounding is monotone): every pair that could be accepted is inside.
#pragma once
#if defined(__HIPCC__)
#include "track.hip"
#else
#include "track_reject.hip"
#endif
#include "cell_grid.hpp"

namespace lmono {

constexpr int kIcpSweeps = 8;                   // cyclic Jacobi sweeps of the 4 x 4 problem (the off-diagonal is exactly 0 on the cases of tests/test_icp_ref_cpu.py)
constexpr float kIcpMaxCorr = 16.0f;
constexpr int kIcpMaxIter = 65536;              // of a handle: the history is kept for every iteration
constexpr int kIcpWords = 26;                   // of IcpSums

// N, Su[3], Sw[3], nine products iu_a * iw_b (|P| < 2^54) as hi = P >> 26 and lo = P - (hi << 26) in [0, 2^26), E.  With n <= 2^28 every word stays below 2^63
struct IcpSums { long long N, Su[3], Sw[3], hi[9], lo[9], E; };
static_assert(sizeof(IcpSums) == 8 * kIcpWords, "IcpSums layout");

struct IcpState {
    double R[9], tau[3];
    double mse_prev;
    long long last_n, last_e;                   // N and E of the last iteration that ran
    int k, status, done, pad;                   // k: iterations run
};

// a centred, in-span coordinate (icp_in_span) in units of 2^-16 m
LMONO_VM_HD long long icp_fix(float c) { return (long long)((double)c * 65536.0); }

// one coordinate of G p: row of a row-major 3 x 4 fp64 transform
LMONO_VM_HD float icp_guess_axis(const double *row, float x, float y, float z)
{
    return (float)(((row[0] * (double)x + row[1] * (double)y) + row[2] * (double)z) + row[3]);
}

// one coordinate of q under the state: row a of R, tau_a, o_a
LMONO_VM_HD float icp_q_axis(const double *row, double tau, float o, float ux, float uy, float uz)
{
    const double v = ((row[0] * (double)ux + row[1] * (double)uy) + row[2] * (double)uz) + tau;
    return (float)((double)o + v);
}

// candidate (d2, x, y, z) before the best so far (bd2, bx, by, bz): nearer, or as near and smaller by x, then y, then z
LMONO_VM_HD bool icp_better(float d2, float x, float y, float z, float bd2, float bx, float by, float bz)
{
    if (d2 != bd2) return d2 < bd2;
    if (x != bx) return x < bx;
    if (y != by) return y < by;
    return z < bz;
}

// what one accepted pair adds: u, w centred and in span, d2 its distance
LMONO_VM_HD void icp_terms(const float u[3], const float w[3], float d2, IcpSums &s)
{
    long long iu[3], iw[3];
    for (int a = 0; a < 3; a++) { iu[a] = icp_fix(u[a]); iw[a] = icp_fix(w[a]); }
    s.N = 1;
    for (int a = 0; a < 3; a++) { s.Su[a] = iu[a]; s.Sw[a] = iw[a]; }
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const long long P = iu[a] * iw[b], hi = P >> 26;
            s.hi[3 * a + b] = hi; s.lo[3 * a + b] = P - hi * 67108864ll;
        }
    s.E = (long long)(uint64_t)((double)d2 * 16777216.0);
}

// R' and tau' from the sums (N >= 3); swept (optional, [16]): Horn's matrix as the sweeps leave it, for the check that they diagonalise it
LMONO_VM_HD void icp_solve(const IcpSums &s, double *R, double *tau, double *swept = nullptr)
{
    const double n = (double)s.N;
    double ub[3], wb[3], S[9];
    for (int a = 0; a < 3; a++) { ub[a] = (double)s.Su[a] / n; wb[a] = (double)s.Sw[a] / n; }
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) S[3 * a + b] = ((double)s.hi[3 * a + b] * 67108864.0 + (double)s.lo[3 * a + b]) - (double)s.Su[a] * wb[b];
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double A[16], V[16];
    A[0] = (Sxx + Syy) + Szz; A[1] = Syz - Szy;         A[2] = Szx - Sxz;           A[3] = Sxy - Syx;
    A[4] = A[1];              A[5] = (Sxx - Syy) - Szz; A[6] = Sxy + Syx;           A[7] = Szx + Sxz;
    A[8] = A[2];              A[9] = A[6];              A[10] = (-Sxx + Syy) - Szz; A[11] = Syz + Szy;
    A[12] = A[3];             A[13] = A[7];             A[14] = A[11];              A[15] = (-Sxx - Syy) + Szz;
    rej_jacobi<4>(A, V, kIcpSweeps);
    if (swept) for (int e = 0; e < 16; e++) swept[e] = A[e];
    int b = 0;
    for (int i = 1; i < 4; i++) if (A[i * 4 + i] > A[b * 4 + b]) b = i;
    double w = V[b], x = V[4 + b], y = V[8 + b], z = V[12 + b];
    const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / nrm; x = x / nrm; y = y / nrm; z = z / nrm;
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
    for (int a = 0; a < 3; a++) tau[a] = (wb[a] - ((R[3 * a] * ub[0] + R[3 * a + 1] * ub[1]) + R[3 * a + 2] * ub[2])) / 65536.0;
}

LMONO_VM_HD void icp_state_init(IcpState &st)
{
    for (int e = 0; e < 9; e++) st.R[e] = (e % 4 == 0) ? 1.0 : 0.0;
    st.tau[0] = st.tau[1] = st.tau[2] = 0.0;
    st.mse_prev = 0.0; st.last_n = 0; st.last_e = 0;
    st.k = 0; st.status = 3; st.done = 0; st.pad = 0;
}

// the end of iteration st.k + 1 from its sums: the new state, the outcome and whether the run is over
LMONO_VM_HD void icp_iterate(IcpState &st, const IcpSums &s, int max_iter, double eps, double mse_eps)
{
    const int k = st.k + 1;
    st.k = k; st.last_n = s.N; st.last_e = s.E;
    if (s.N < 3) { st.status = 3; st.done = 1; return; }
    double R[9], tau[3];
    icp_solve(s, R, tau);
    double dt = 0.0, dR = 0.0;
    for (int a = 0; a < 3; a++) { const double d = tau[a] - st.tau[a]; dt = dt + d * d; }
    for (int e = 0; e < 9; e++) { const double d = R[e] - st.R[e]; dR = dR + d * d; }
    for (int e = 0; e < 9; e++) st.R[e] = R[e];
    for (int a = 0; a < 3; a++) st.tau[a] = tau[a];
    const double mse = (double)s.E / (double)s.N / 16777216.0, mse_prev = st.mse_prev;
    st.mse_prev = mse;
    if (dt < eps && dR < eps) { st.status = 0; st.done = 1; }
    else if (mse_eps > 0.0 && k >= 2 && fabs(mse - mse_prev) < mse_eps) { st.status = 2; st.done = 1; }
    else if (k == max_iter) { st.status = 1; st.done = 1; }
}

// the result: [R | ((double)o + tau) - R o] composed with the guess G, row-major 3 x 4
LMONO_VM_HD void icp_transform(const IcpState &st, const float o[3], const double *G, double *T)
{
    for (int a = 0; a < 3; a++) {
        const double *r = st.R + 3 * a;
        const double t = ((double)o[a] + st.tau[a]) - ((r[0] * (double)o[0] + r[1] * (double)o[1]) + r[2] * (double)o[2]);
        for (int b = 0; b < 3; b++) T[4 * a + b] = (r[0] * G[b] + r[1] * G[4 + b]) + r[2] * G[8 + b];
        T[4 * a + 3] = ((r[0] * G[3] + r[1] * G[7]) + r[2] * G[11]) + t;
    }
}

// The default cell for max_corr D at 2 rings: the smallest float32 h >= D / 1.75f with sor_rho(2, h) >= D.  D / 1.75f alone misses the bound by one ulp
// for about 5 % of D (1.75f * (D / 1.75f) rounds below D whenever D's mantissa lies in [1.75, 2): 0.95, 1.9, 3.8 ...); one or two steps up repair it.
// A tuning value: it cannot change a result.
inline float icp_default_cell(float max_corr)
{
    float h = max_corr / 1.75f;
    for (int k = 0; k < 4 && !(sor_rho(2, h) >= max_corr); k++) h = std::nextafterf(h, INFINITY);
    return h;
}

// bounds of the parameters (the create function and icp_test refuse alike)
LMONO_VM_HD bool icp_params_ok(float max_corr, int max_iter, double eps, double mse_eps, float cell, int max_rings)
{
    if (!(max_corr > 0.0f && max_corr <= kIcpMaxCorr) || max_iter < 1 || max_iter > kIcpMaxIter || !(eps >= 0.0) || !(mse_eps >= 0.0)) return false;
    if (!(cell > 0.0f) || !(1.0f / cell > 0.0f) || !(1.0f / cell <= 3.0e38f) || max_rings < 1 || max_rings > kSorMaxRings) return false;
    return sor_rho(max_rings, cell) >= max_corr;
}

} // namespace lmono
