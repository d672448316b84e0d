// trust_region.hpp -- the 6-DoF solver core of the two LiDAR solves: k_lm_solve (odometry.hip, laserOdometry) and k_map_solve
// (mapping.hip, laserMapping).  The sums of a linearisation (H 21 | g 6 | cost, 28 doubles), the packed 6 x 6 Cholesky solve, the
// pose's plus operation, and TrustRegion: Ceres' trust-region loop (Levenberg-Marquardt, DENSE_QR restated on the 6 x 6 normal
// equations) cut open at its evaluations, which are the kernels' own.  The oracle's counterpart is lo_lm_solve.
// No GPU intrinsic in here: tests/test_trust_region_cpu.py compiles this header for the host and drives the branches no scene reaches.
//
// Contraction to FMA is allowed in accumulate_row and chol_solve6_packed alone (their pragmas); everything else in this file is
// compiled as the translation unit is, -ffp-contract=off, in both kernels.
#pragma once

#include <float.h>
#include <math.h>

#if defined(__HIPCC__)
#define TR_FN __device__ __forceinline__
#else
#define TR_FN inline
#endif

namespace lmono {

struct LmAcc { double H[21]; double g[6]; double cost; };

TR_FN void accumulate_row(LmAcc &a, const double *J, double r)
{
#pragma clang fp contract(fast)
    int t = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        a.g[i] += J[i] * r;
#pragma unroll
        for (int j = i; j < 6; j++) a.H[t++] += J[i] * J[j];
    }
}

TR_FN void huber(double s, double &rho0, double &rho1)
{
    const double a = 0.1, bb = 0.1 * 0.1;
    if (s > bb) {
        const double r = sqrt(s);
        rho0 = 2.0 * a * r - bb;
        rho1 = a / r;
        if (rho1 < DBL_MIN) rho1 = DBL_MIN;
    } else { rho0 = s; rho1 = 1.0; }
}

// entry (i, j) of a symmetric 6 x 6 matrix stored as its upper triangle row by row (the order of accumulate_row)
TR_FN int sym6(int i, int j) { const int a = i < j ? i : j, b = i < j ? j : i; return a * 6 - a * (a - 1) / 2 + (b - a); }

// Cholesky factorisation and the two substitutions on the LOWER triangle stored row by row (entry (i, j), j <= i, at i (i + 1) / 2 + j),
// in place: 21 doubles instead of two 6 x 6 arrays.
// Round 4: the 27 divisions by the factor's diagonal are multiplications by its six reciprocals (an fp64 division is ~35 instructions on the one wave
// per SIMD that runs a chain's solve, and every thread of the workgroup runs this redundantly four times per launch: ~24 k of a launch's ~126 k cycles).
// Same factorisation to rounding; the solve's parity bar is 1e-9 against the oracle's loop.
TR_FN bool chol_solve6_packed(double *L, const double *bvec, double *xo)
{
#pragma clang fp contract(fast)
    double inv[6];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double s = L[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            if (i == j) { if (!(s > 0.0)) return false; const double d = sqrt(s); L[i * (i + 1) / 2 + i] = d; inv[i] = 1.0 / d; }
            else L[i * (i + 1) / 2 + j] = s * inv[j];
        }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = bvec[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[i * (i + 1) / 2 + k] * y[k];
        y[i] = s * inv[i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s -= L[k * (k + 1) / 2 + i] * xo[k];
        xo[i] = s * inv[i];
    }
    return true;
}

TR_FN void manifold_plus(const double *x, const double *d, double *o)
{
    const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (nd > 0.0) {
        const double sc = sin(nd) / nd;
        const double ax = sc * d[0], ay = sc * d[1], az = sc * d[2], aw = cos(nd);
        const double bx = x[0], by = x[1], bz = x[2], bw = x[3];
        o[3] = aw * bw - ax * bx - ay * by - az * bz;
        o[0] = aw * bx + ax * bw + ay * bz - az * by;
        o[1] = aw * by + ay * bw + az * bx - ax * bz;
        o[2] = aw * bz + az * bw + ax * by - ay * bx;
    } else { o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; o[3] = x[3]; }
    o[4] = x[4] + d[3]; o[5] = x[5] + d[4]; o[6] = x[6] + d[5];
}

TR_FN double norm7(const double *x)
{
    double s = 0.0;
    for (int i = 0; i < 7; i++) s += x[i] * x[i];
    return sqrt(s);
}

// The three steps of the trust-region loop between two evaluations.  The caller evaluates: the accepted linearisation is in s_cur, a
// candidate's sums in s_sum (both 28 doubles: H as accumulate_row leaves it | g | cost), x is the accepted pose.
//     if (tr.begin(s_cur, x))
//         for (;;) {
//             const int ctl = tr.propose(s_cur, x, cand);
//             if (ctl == 2) break;
//             s_sum <- sums at cand, with its Jacobian (ctl 0) or the cost alone (ctl 1)
//             if (!tr.judge(s_sum, s_cur, x, cand, take)) break;
//         }
// take() makes s_sum the accepted linearisation (s_cur <- s_sum, with whatever barriers the caller's threads need).
// kRecipRadius: the damping term is diag * (1 / radius) (k_lm_solve) or diag / radius (k_map_solve, the oracle's form); each kernel
// keeps the arithmetic it was tested with.
template <bool kRecipRadius>
struct TrustRegion {
    static constexpr double function_tol = 1e-6, gradient_tol = 1e-10, parameter_tol = 1e-8;
    static constexpr double min_rel_decrease = 1e-3, min_diag = 1e-6, max_diag = 1e32, max_radius = 1e16, min_radius = 1e-32;

    double radius = 1e4, decrease_factor = 2.0, x_cost = 0.0, x_norm = 0.0, model_change = 0.0;
    double scale[6], diag[6];      // set by begin / by the first propose (reuse_diagonal starts false)
    bool reuse_diagonal = false;
    int invalid_steps = 0, iter = 0;
    int max_iter;                  // ceres max_num_iterations

    TR_FN explicit TrustRegion(int max_iterations) : max_iter(max_iterations) {}

    TR_FN bool last() const { return iter == max_iter; }      // the step proposed last gets no iteration after it

    TR_FN static double max_abs_gradient(const double *s)
    {
        double gmax = 0.0;
        for (int i = 0; i < 6; i++) gmax = fmax(gmax, fabs(s[21 + i]));
        return gmax;
    }

    // false: the gradient at the start is below tolerance already
    TR_FN bool begin(const double *s_cur, const double *x)
    {
        x_cost = s_cur[27];
        if (!(max_abs_gradient(s_cur) > gradient_tol)) return false;
        x_norm = norm7(x);
        for (int i = 0; i < 6; i++) scale[i] = 1.0 / (1.0 + sqrt(s_cur[sym6(i, i)]));
        return true;
    }

    // The next candidate pose.  0: evaluate it with its Jacobian (it is accepted almost always, and then this is the linearisation of the
    // next iteration -- the same numbers a separate pass would give), 1: its cost only (the last iteration), 2: finished.
    TR_FN int propose(const double *s_cur, const double *x, double *cand)
    {
        while (iter < max_iter) {
            iter++;
            double gs[6], A[21], stepv[6];
            // lower triangle of A = Hs = H scale_i scale_j, then + diag / radius on the diagonal
#pragma unroll
            for (int i = 0; i < 6; i++) {
                gs[i] = s_cur[21 + i] * scale[i];
#pragma unroll
                for (int j = 0; j <= i; j++) A[i * (i + 1) / 2 + j] = s_cur[sym6(i, j)] * scale[i] * scale[j];
            }
            if (!reuse_diagonal)
                for (int i = 0; i < 6; i++) { double d = A[i * (i + 1) / 2 + i]; d = d < min_diag ? min_diag : d; d = d > max_diag ? max_diag : d; diag[i] = d; }
            if (kRecipRadius) { const double ir = 1.0 / radius; for (int i = 0; i < 6; i++) A[i * (i + 1) / 2 + i] += diag[i] * ir; }
            else for (int i = 0; i < 6; i++) A[i * (i + 1) / 2 + i] += diag[i] / radius;
            bool ok = chol_solve6_packed(A, gs, stepv);
            for (int i = 0; i < 6; i++) if (!isfinite(stepv[i])) ok = false;
            model_change = 0.0;
            if (ok) {
                for (int i = 0; i < 6; i++) stepv[i] = -stepv[i];
                double dg = 0.0, dHd = 0.0;
                for (int i = 0; i < 6; i++) { dg += stepv[i] * gs[i]; for (int j = 0; j < 6; j++) dHd += stepv[i] * (s_cur[sym6(i, j)] * scale[i] * scale[j]) * stepv[j]; }
                model_change = -(dg + 0.5 * dHd);
            }
            if (!ok || !(model_change > 0.0)) {
                if (++invalid_steps >= 5) return 2;
                radius *= 0.5; reuse_diagonal = true;
                continue;
            }
            invalid_steps = 0;
            double delta[6];
            for (int i = 0; i < 6; i++) delta[i] = stepv[i] * scale[i];
            manifold_plus(x, delta, cand);
            return last() ? 1 : 0;
        }
        return 2;
    }

    // The candidate's sums are in s_sum: the two tolerance exits, then accept (x <- cand; take(), unless nothing after this step is
    // used) or reject, and the radius rule.  false: the solve is finished.
    template <class Take>
    TR_FN bool judge(const double *s_sum, const double *s_cur, double *x, const double *cand, Take take)
    {
        const double cand_cost = s_sum[27];
        double sn = 0.0;
        for (int i = 0; i < 7; i++) sn += (x[i] - cand[i]) * (x[i] - cand[i]);
        sn = sqrt(sn);
        if (sn <= parameter_tol * (x_norm + parameter_tol)) return false;
        if (fabs(x_cost - cand_cost) <= function_tol * x_cost) return false;
        const double rel = (x_cost - cand_cost) / model_change;
        if (rel > min_rel_decrease) {
            for (int i = 0; i < 7; i++) x[i] = cand[i];
            if (last()) return false;
            x_norm = norm7(x);
            x_cost = cand_cost;
            take();
            const double tt = 2.0 * rel - 1.0;
            double den = 1.0 - tt * tt * tt;
            if (den < 1.0 / 3.0) den = 1.0 / 3.0;
            radius = radius / den;
            if (radius > max_radius) radius = max_radius;
            decrease_factor = 2.0; reuse_diagonal = false;
            if (max_abs_gradient(s_cur) <= gradient_tol) return false;
        } else {
            radius = radius / decrease_factor; decrease_factor *= 2.0; reuse_diagonal = true;
        }
        return !(radius <= min_radius);
    }
};

}  // namespace lmono
