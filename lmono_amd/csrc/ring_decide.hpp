// lmono_amd/csrc/ring_decide.hpp -- the two decisions k_ring_tag takes per point (ring id, half sweep), without an arctangent.
// Host and device compile the same IEEE float operations (-ffp-contract=off on both sides), so a CPU program runs the identical decision
// code (tests/ring_decide_check.cpp).  The one device-specific input, the reciprocal square root, is an argument.
//
// Both decisions choose between alternatives of the fp64 reference form (det_atan / det_atan2, oracle/lo_scanreg.c).  A cheap evaluation
// with a proven error bound settles every point that is farther than a guard (20x the bound) from every place where the reference's
// answer changes; the others take the reference form itself.
//
// 1  Elevation.  t = z * rs with rs ~ 1 / sqrt(q2), q2 = x x + y y in float (the reference divides by the square root of the same float).
//    angle = t P(t^2) in degrees, P of degree 5: the interpolant of atan(t) / t at the Chebyshev nodes of [0, 0.6275^2] in t^2.
//    Valid for |t| <= 0.6275 = tan 32.1 deg; every supported sensor discards outside a window inside that (16 lines: -18 .. 16 deg,
//    32 lines: -32 .. 12, 64 lines: -18.08 .. 2, the lower end being where id > 50 begins; -24.33 lies behind it).  A t outside the
//    window widened by at least 0.05 deg is discarded from a comparison of t alone.
//    Error of the angle against the reference's float angle, in degrees:
//      polynomial against atan in exact arithmetic                                          1.7e-6
//      its evaluation in float (12 roundings, the last ones at 32 deg: ulp 3.8e-6)          4.0e-6   (measured with the line above: 4.9e-6)
//      t: rs within 1 ulp (v_rsq_f32) and one product, relative 1.8e-7; d angle = t / (1 + t^2) * 1.8e-7 rad <= 7.8e-8 rad   4.5e-6
//      the reference's own rounding of its angle to float (half an ulp at 32 deg)           1.9e-6
//      the map to the ring variable v in float where the reference uses double: 4 roundings at v <= 64 (ulp 3.8e-6),
//      through the smallest slope 1 / 2                                                     3.1e-5   (16 lines; 64 lines: slope 2, 7.6e-6)
//    (tests/ring_decide_check.cpp steps float by float across every guard band and finds no fast answer that differs from the exact one.)
//    Sum < 4.5e-5 < 1e-4 deg: the bound.  kRingGuardDeg = 2e-3 = 20x the bound, unchanged.
// 2  Ring id.  ring_of is piecewise linear in the angle and truncates towards zero: with v the mapped variable of the applicable branch its
//    answer changes where v passes a non-zero integer (0 is no threshold: (int) maps (-1, 1) to 0), at the 64-line branch switch -8.83
//    and at the 64-line limit 2 deg.  id < 0, id > n - 1 and id > 50 are integers of v.  The fast answer is (int)v when v is farther than
//    guard * slope (the larger slope where there are two) from the nearest integer (or that integer is 0) and, for 64 lines, the angle farther than the guard from -8.83 and 2.
// 3  Half sweep.  With ori the angle of (x, -y) and startOri that of the first valid point (x0, -y0), the reference's wrapped difference
//    d = ori - startOri lies in [-pi / 2, 3 pi / 2] and past_half <=> d > pi: the third quadrant relative to the start direction,
//    dot = x ux + y uy < 0 and cross = uy x - ux y < 0 with (ux, uy) = (x0, y0) / rho0.  The answer changes at d = pi (cross = 0, dot < 0)
//    and at d = 3 pi / 2 = -pi / 2 (dot = 0, cross < 0); |cross| / rho and |dot| / rho are the sine of the distance to them.
//    Error of that distance against the reference's float arithmetic, in radians:
//      dot, cross: two products and a sum, <= 3 * 2^-24 rho                                 1.8e-7
//      (ux, uy) rounded to float                                                            0.9e-7
//      rho = q2 * rs in the comparison: relative 2e-7 of a guard                            < 1e-10
//      the reference's float startOri and ori (half an ulp at pi)                           2 * 1.2e-7
//      its o1 +- 2 pi rounded to float (values up to 3 pi: half an ulp 4.8e-7)              4.8e-7
//      its float subtraction o1 - startOri (results up to 3 pi / 2: half an ulp 2.4e-7)     2.4e-7
//    Sum < 1.3e-6 < 2e-6 rad: the bound.  kHalfGuardRad = 4e-5 = 20x the bound, unchanged.
//    A first point with x0 = y0 = 0 has startOri = -atan2(0, 0) = 0: start direction (1, 0).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LMONO_HD __host__ __device__ __forceinline__
#else
#define LMONO_HD inline
#endif

namespace lmono {

constexpr float kRingGuardDeg = 2e-3f;         // 20x the angle's error bound (1e-4 deg)
constexpr float kHalfGuardRad = 4e-5f;         // 20x the bound of the half test (2e-6 rad)
constexpr float kRingQ2Min = 1e-30f, kRingQ2Max = 1e30f;      // x x + y y outside: the reference form (x = y = 0; rho = q2 * rs would be inf * 0)

// atan(t) in degrees for |t| <= 0.6275, plain float operations
LMONO_HD float ring_elev_deg(float t)
{
    const float u = t * t;
    float p = -2.153733492e+00f;
    p = p * u + 5.257353783e+00f;
    p = p * u + -7.979190826e+00f;
    p = p * u + 1.144106770e+01f;
    p = p * u + -1.909799767e+01f;
    p = p * u + 5.729577637e+01f;
    return t * p;
}

// The reference's map from the elevation a (deg) to the ring variable v, one form for the three sensors: v = (c0 - a) m + c1 with the
// constants of the upper branch for a >= sw and of the lower branch below (16 and 32 lines have one branch: sw = -inf; (a + 15) / 2 + 0.5
// is (-15 - a) (-0.5) + 0.5 bit for bit).  The same for every point of a launch: made once, held in scalar registers.
struct RingMap {
    float t_lo, t_hi;              // t outside: discarded without the polynomial (at least 0.05 deg outside the window of kept elevations)
    float sw, c0[2], m[2], c1[2];  // [0] upper branch, [1] lower branch
    float gs;                      // guard in v: guard * the larger |m| (64 lines: 3 guards for both branches, 1.5 guards of elevation in the lower one)
    float g_a;                     // guard of the thresholds in a itself: a_max and sw (0: there are none)
    float a_max;                   // above: discarded whatever v is
    float hi;                      // v in (-1, hi) is a ring
};

LMONO_HD RingMap ring_map(int n_lines)
{
    RingMap r;
    if (n_lines == 16) {
        r.t_lo = -0.3265f; r.t_hi = 0.2885f;                              // -18.08 / 16.09 deg
        r.sw = -INFINITY; r.c0[0] = r.c0[1] = -15.0f; r.m[0] = r.m[1] = -0.5f; r.c1[0] = r.c1[1] = 0.5f; r.gs = kRingGuardDeg * 0.5f;
        r.g_a = 0.0f; r.a_max = INFINITY; r.hi = 16.0f;
    } else if (n_lines == 32) {
        r.t_lo = -0.627f; r.t_hi = 0.2145f;                               // -32.09 / 12.10 deg
        r.sw = -INFINITY; r.c0[0] = r.c0[1] = -30.666666f; r.m[0] = r.m[1] = -0.75f; r.c1[0] = r.c1[1] = 0.0f; r.gs = kRingGuardDeg * 0.75f;
        r.g_a = 0.0f; r.a_max = INFINITY; r.hi = 32.0f;
    } else {
        r.t_lo = -0.328f; r.t_hi = 0.036f;                                // -18.16 (id > 50 from -18.08 on) / 2.06 deg
        r.sw = -8.83f;
        r.c0[0] = 2.0f; r.m[0] = 3.0f; r.c1[0] = 0.5f; r.gs = kRingGuardDeg * 3.0f;               // (2 - a) 3 + 0.5
        r.c0[1] = -8.83f; r.m[1] = 2.0f; r.c1[1] = 32.5f;                                         // 32 + (-8.83 - a) 2 + 0.5
        r.g_a = kRingGuardDeg; r.a_max = 2.0f; r.hi = 51.0f;
    }
    return r;
}

// Ring id from t = z * rs.  true: decided (id, or -1 = discarded); false: within the guard of a threshold, take the reference form.
// Written without exits: on the device every comparison becomes a lane mask and every choice a select (with an exit per test the kernel
// issued more scalar instructions, 0.81 G per step, than vector ones; without them 0.34 G: profiles/r14/NOTES.md).
// A t outside the window makes the polynomial meaningless (or NaN): `out` decides alone then.
LMONO_HD bool ring_fast(float t, const RingMap &r, int &id)
{
    const float a = ring_elev_deg(t);
    const bool out = !((t > r.t_lo) & (t < r.t_hi));
    const float vu = (r.c0[0] - a) * r.m[0] + r.c1[0], vl = (r.c0[1] - a) * r.m[1] + r.c1[1];      // both branches: six operations on constants, one select
    const float v = a >= r.sw ? vu : vl;
    const float k = rintf(v);
    const bool near = (fminf(fabsf(a - r.a_max), fabsf(a - r.sw)) < r.g_a) | ((fabsf(v - k) < r.gs) & (k != 0.0f));
    const bool keep = !out & !(a > r.a_max) & (v > -1.0f) & (v < r.hi);
    id = keep ? (int)(keep ? v : 0.0f) : -1;
    return out | !near;
}

// unit vector of the sweep's start direction from the first valid point
LMONO_HD void ring_start_dir(float x0, float y0, float &ux, float &uy)
{
    const double q = (double)x0 * (double)x0 + (double)y0 * (double)y0;
    ux = 1.0f; uy = 0.0f;
    if (q > 0.0) {
        const double r = sqrt(q);
        ux = (float)((double)x0 / r); uy = (float)((double)y0 / r);
    }
}

// Half-sweep test of (x, y) at horizontal range rho against the start direction.  true: decided (past); false: take the reference form.
LMONO_HD bool half_fast(float x, float y, float rho, float ux, float uy, bool &past)
{
    const float dot = x * ux + y * uy, cross = uy * x - ux * y;
    const float g = kHalfGuardRad * rho;
    const bool dn = dot < 0.0f, cn = cross < 0.0f;
    past = dn & cn;
    return !((dn & (fabsf(cross) < g)) | (cn & (fabsf(dot) < g)));
}

// Both decisions of one valid point, rs ~ 1 / sqrt(x x + y y) within 1 ulp.  true: decided (id, or -1 = discarded; past_half, false for a
// discarded point); false: take the reference forms for this point.
LMONO_HD bool ring_half_fast(float x, float y, float z, float q2, float rs, const RingMap &r, float ux, float uy, int &id, bool &past_half)
{
    bool past;
    const bool in_q = (q2 > kRingQ2Min) & (q2 < kRingQ2Max);
    const bool ring_ok = ring_fast(z * rs, r, id);
    const bool half_ok = half_fast(x, y, q2 * rs, ux, uy, past);
    past_half = past & (id >= 0);
    return in_q & ring_ok & ((id < 0) | half_ok);
}

} // namespace lmono
