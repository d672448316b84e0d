// Curvature and neighbour-gap flags of a sector from the registers of a wave, host and device (tests/curv_window_check.cpp builds this
// header with g++ and runs it over 64 modelled lanes).
//
// scanRegistration's curvature of point i is the squared length of (sum of the ten neighbours i - 5 .. i + 5) - 10 p[i], and its gap
// flag says that the step to the next point of the cloud is long:
//   dx = x[i-5] + x[i-4] + x[i-3] + x[i-2] + x[i-1] - 10 x[i] + x[i+1] + x[i+2] + x[i+3] + x[i+4] + x[i+5]     (left to right; dy, dz alike)
//   cv = dx dx + dy dy + dz dz
//   gap[i] = (double)(gx gx + gy gy + gz gz) > 0.05,   g = p[i+1] - p[i]
// in float, uncontracted.  k_curvature evaluates exactly this per point of a whole cloud.  k_select needs it for the elements of one
// sector at a time, and a wave of k_select holds M consecutive points per lane: the eleven values around an element are registers of
// its own lane, the last five of the lane before and the first five of the lane behind (M >= 5: one neighbour lane is enough).
//
// Layout: lane L owns the M points L M .. L M + M - 1 counted from the sector's first element.  Position p of a lane is its point p;
// p = -5 .. -1 are the last five of the lane before, p = M .. M + 4 the first five of the lane behind.  The wave has two ends: what
// lane 0 sees before itself and what lane 63 sees behind itself comes from five `halo` points that those two lanes hold themselves
// (lane 0: the five points before the sector, lane 63: the five points behind its own; the other lanes' halo is not read).
//
// The curvature goes one coordinate at a time: cv is a sum of three squares added in the order x, y, z, the order of the expression
// above, so a pass per coordinate keeps one window of M + 10 values in registers instead of three.  The gap flags come first and
// leave one bit mask behind.
//
// The lanes are a policy L over the value types (float / unsigned int on the device, 64 of them side by side in the host model):
//   L::before(v, old)   v of the lane before; lane 0 keeps old        (DPP wave_shr:1 with the old value as the destination)
//   L::behind(v, old)   v of the lane behind; lane 63 keeps old       (DPP wave_shl:1)
//   L::bits             the type that holds one bit mask per lane
// and curv_gap_flag is overloaded for the value type.
#pragma once

#if defined(__HIPCC__)
#define LMONO_CW_HD __host__ __device__ __forceinline__
#define LMONO_CW_UNROLL _Pragma("unroll")
#else
#define LMONO_CW_HD inline
#define LMONO_CW_UNROLL
#endif

namespace lmono {

constexpr int kCurvReach = 5;      // neighbours on either side of a point

// one coordinate's term of the curvature of the element at w[5]: operands and order are k_curvature's
template <class T>
LMONO_CW_HD T curv_diff(const T *w)
{
    return w[0] + w[1] + w[2] + w[3] + w[4] - 10 * w[5] + w[6] + w[7] + w[8] + w[9] + w[10];
}

// the gap flag of a point from the step to the next one
LMONO_CW_HD bool curv_gap_long(float s) { return (double)s > 0.05; }      // s: the squared step, gx gx + gy gy + gz gz
LMONO_CW_HD unsigned int curv_gap_flag(float gx, float gy, float gz) { return curv_gap_long(gx * gx + gy * gy + gz * gz) ? 1u : 0u; }

// The gap flags of the five halo points (bit d: halo point d) from the halo and the point that stands behind it, h*[5]: lane 0's own
// first point (its halo ends where the sector begins).  Lane 63's halo continues its own points, and the flag of its fifth halo point
// is one of the bits that nobody reads: whatever stands in its h*[5] will do.
template <class U, class T>
LMONO_CW_HD U curv_halo_flags(const T (&hx)[kCurvReach + 1], const T (&hy)[kCurvReach + 1], const T (&hz)[kCurvReach + 1])
{
    U hb = curv_gap_flag(hx[1] - hx[0], hy[1] - hy[0], hz[1] - hz[0]);
    LMONO_CW_UNROLL
    for (int d = 1; d < kCurvReach; d++) hb = hb | (curv_gap_flag(hx[d + 1] - hx[d], hy[d + 1] - hy[d], hz[d + 1] - hz[d]) << d);
    return hb;
}

// The lane's window of gap flags: bit k = gap flag of position k - 5, k < M + 9 (the step from position M + 3 to M + 4 is the last a
// window can show; the bits from M + 9 on are not flags of anything and no reader looks at them).
// o*: the lane's M points; h*0: its first halo point (what stands behind lane 63's last point); hb: curv_halo_flags.
template <int M, class L, class T>
LMONO_CW_HD typename L::bits curv_gap_window(const L &lanes, const T (&ox)[M], const T (&oy)[M], const T (&oz)[M],
                                             const T &hx0, const T &hy0, const T &hz0, const typename L::bits &hb)
{
    static_assert(M >= kCurvReach, "one neighbour lane on either side must hold the five neighbours");
    typedef typename L::bits U;
    const T nx = lanes.behind(ox[0], hx0), ny = lanes.behind(oy[0], hy0), nz = lanes.behind(oz[0], hz0);      // the point behind the lane's last
    U own = curv_gap_flag(ox[1] - ox[0], oy[1] - oy[0], oz[1] - oz[0]);
    LMONO_CW_UNROLL
    for (int m = 1; m < M - 1; m++) own = own | (curv_gap_flag(ox[m + 1] - ox[m], oy[m + 1] - oy[m], oz[m + 1] - oz[m]) << m);
    own = own | (curv_gap_flag(nx - ox[M - 1], ny - oy[M - 1], nz - oz[M - 1]) << (M - 1));
    const U prev = lanes.before(own, hb << (M - kCurvReach));              // lane 0: the halo's flags, where the lane before would have its last five
    const U next = lanes.behind(own, hb);                                  // lane 63: the halo's flags
    return (prev >> (M - kCurvReach)) | (own << kCurvReach) | (next << (M + kCurvReach));
}

// One coordinate's window of a lane, positions -5 .. M + 4: cv[m] = curvature of point m so far (first: this is x, the sums start).
template <int M, class T>
LMONO_CW_HD void curv_window_accum(const T (&w)[M + 2 * kCurvReach], bool first, T (&cv)[M])
{
    LMONO_CW_UNROLL
    for (int m = 0; m < M; m++) {
        const T dc = curv_diff(w + m);
        const T dd = dc * dc;
        cv[m] = first ? dd : cv[m] + dd;
    }
}

// One coordinate of the lane's M points (own) and of its halo: cv[m] = curvature of point m so far.  first: this is x, the sums start;
// otherwise they go on.
template <int M, class L, class T>
LMONO_CW_HD void curv_window_coord(const L &lanes, const T (&own)[M], const T (&halo)[kCurvReach], bool first, T (&cv)[M])
{
    static_assert(M >= kCurvReach, "one neighbour lane on either side must hold the five neighbours");
    T w[M + 2 * kCurvReach];
    LMONO_CW_UNROLL
    for (int m = 0; m < M; m++) w[m + kCurvReach] = own[m];
    LMONO_CW_UNROLL
    for (int d = 0; d < kCurvReach; d++) {
        w[d] = lanes.before(own[M - kCurvReach + d], halo[d]);              // point M - 5 + d of the lane before
        w[M + kCurvReach + d] = lanes.behind(own[d], halo[d]);              // point d of the lane behind
    }
    curv_window_accum<M>(w, first, cv);
}

} // namespace lmono
