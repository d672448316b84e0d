// tests/ring_decide_check.cpp -- host proof harness of lmono_amd/csrc/ring_decide.hpp (built and run by tests/test_ring_decide_cpu.py).
// The decision code k_ring_tag runs per point is compiled here for the CPU and compared with the exact decision as the oracle's C
// restatement evaluates it (oracle/lo_scanreg.c: ring_id and the half-sweep wrap, restated below over oracle/lo_det_math.h).
//   wrong         the fast path answered and the answer differs from the exact one                                  must be 0
//   far_fallback  the fast path asked for the exact form although the point is more than 2 guards from every threshold   must be 0
// Every input is run with the reciprocal square root correctly rounded and moved by one ulp in both directions (the documented error
// of v_rsq_f32), which moves t = z * rs and rho = q2 * rs with it.
// Build: g++ -O2 -ffp-contract=off.
#include "../lmono_amd/csrc/ring_decide.hpp"
#include "../oracle/lo_det_math.h"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
using namespace lmono;

static int ring_id(float angle, int n_scans, int *discard)        // oracle/lo_scanreg.c, word for word
{
    int id = 0;
    *discard = 0;
    if (n_scans == 16) {
        id = (int)((double)((angle + 15.0f) / 2.0f) + 0.5);
        if (id > n_scans - 1 || id < 0) *discard = 1;
    } else if (n_scans == 32) {
        id = (int)(((double)angle + 92.0 / 3.0) * 3.0 / 4.0);
        if (id > n_scans - 1 || id < 0) *discard = 1;
    } else { /* 64 */
        if ((double)angle >= -8.83)
            id = (int)((double)(2.0f - angle) * 3.0 + 0.5);
        else
            id = n_scans / 2 + (int)((-8.83 - (double)angle) * 2.0 + 0.5);
        if ((double)angle > 2.0 || (double)angle < -24.33 || id > 50 || id < 0) *discard = 1;
    }
    return id;
}

static bool exact_half(float x, float y, float startOri)
{
    float ori = (float)(-lo_atan2((double)y, (double)x));
    if ((double)ori < (double)startOri - LO_PI / 2.0) ori = (float)((double)ori + 2.0 * LO_PI);
    else if ((double)ori > (double)startOri + LO_PI * 3.0 / 2.0) ori = (float)((double)ori - 2.0 * LO_PI);
    return (double)(ori - startOri) > LO_PI;
}

// k_ring_tag's per-point decision with the reciprocal square root it is given: 0 = take the exact forms, 1 = decided
static int fast_decide(float x, float y, float z, int n_lines, float ux, float uy, float rs, int &id, bool &past)
{
    return ring_half_fast(x, y, z, x * x + y * y, rs, ring_map(n_lines), ux, uy, id, past) ? 1 : 0;
}

// floats in order: a monotone integer key
static int64_t fkey(float f) { int32_t b; std::memcpy(&b, &f, 4); return b < 0 ? -(int64_t)(b & 0x7fffffff) : (int64_t)b; }
static float fval(int64_t k) { int32_t b = k < 0 ? (int32_t)(0x80000000u | (uint32_t)(-k)) : (int32_t)k; float f; std::memcpy(&f, &b, 4); return f; }

static long long n_checked = 0, n_fast = 0, n_fallback = 0, n_wrong = 0, n_far_fallback = 0, n_printed = 0;

static std::vector<double> ring_thresholds(int n_lines)        // elevations (deg) where ring_id changes its answer
{
    std::vector<double> t;
    if (n_lines == 16) { t.push_back(-18.0); for (int k = 1; k <= 16; k++) t.push_back(2.0 * k - 16.0); }
    else if (n_lines == 32) { t.push_back(-32.0); for (int k = 1; k <= 32; k++) t.push_back(k * 4.0 / 3.0 - 92.0 / 3.0); }
    else {
        t.push_back(2.0); t.push_back(-8.83);
        for (int k = 1; k <= 32; k++) t.push_back(2.0 - (k - 0.5) / 3.0);              // upper branch: (2 - a) 3 + 0.5 = k
        for (int k = 1; k <= 19; k++) t.push_back(-8.83 - (k - 0.5) / 2.0);            // lower branch: 32 + (int)((-8.83 - a) 2 + 0.5), 51 at -18.08
    }
    return t;
}

static void check_ring(float x, float y, float z, int n_lines, const std::vector<double> &thr)
{
    const float q2 = x * x + y * y;
    const float rs0 = (float)(1.0 / sqrt((double)q2));
    const double ad = lo_atan((double)z / sqrt((double)q2)) * 180.0 / LO_PI;         // the reference's angle is this, rounded to float
    int discard;
    int want = ring_id((float)ad, n_lines, &discard);
    if (discard) want = -1;
    double dist = 1e9;
    for (double t : thr) dist = fmin(dist, fabs(ad - t));
    // below the last threshold / above the first everything is discarded: no further threshold there
    const bool far = dist > 2.0 * (double)kRingGuardDeg;
    const float rsv[3] = { rs0, nextafterf(rs0, 0.0f), nextafterf(rs0, INFINITY) };
    const RingMap map = ring_map(n_lines);
    for (int v = 0; v < 3; v++) {
        int id;
        n_checked++;
        const bool decided = ring_fast(z * rsv[v], map, id);
        if (decided) n_fast++; else n_fallback++;
        const bool wrong = decided && id != want, ff = !decided && far;
        n_wrong += wrong; n_far_fallback += ff;
        if ((wrong || ff) && n_printed++ < 20)
            std::printf("ring n=%d x=%.9g y=%.9g z=%.9g rs%+d angle=%.9g: %s fast=%d exact=%d\n", n_lines, x, y, z, v == 0 ? 0 : (v == 1 ? -1 : 1), ad, wrong ? "WRONG" : "FAR FALLBACK", id, want);
    }
}

// z from lo to hi: every float when there are at most `all` of them, otherwise every float within `win` of lo, hi and the marks, and a stride between
static void sweep_z(float x, float y, float lo, float hi, const float *marks, int n_marks, int n_lines, const std::vector<double> &thr, int64_t all, int64_t win, int64_t n_stride)
{
    const int64_t k0 = fkey(lo), k1 = fkey(hi);
    if (k1 - k0 <= all) { for (int64_t k = k0; k <= k1; k++) check_ring(x, y, fval(k), n_lines, thr); return; }
    for (int m = -2; m < n_marks; m++) {
        const int64_t c = m == -2 ? k0 : (m == -1 ? k1 : fkey(marks[m]));
        for (int64_t k = c - win; k <= c + win; k++) check_ring(x, y, fval(k), n_lines, thr);
    }
    const int64_t step = (k1 - k0) / n_stride + 1;
    for (int64_t k = k0; k <= k1; k += step) check_ring(x, y, fval(k), n_lines, thr);
}

static void elevation_sweeps()
{
    const float rhos[5] = { 0.6f, 3.7f, 20.0f, 77.3f, 200.0f };
    const int lines[3] = { 16, 32, 64 };
    for (int li = 0; li < 3; li++) {
        const int n_lines = lines[li];
        const std::vector<double> thr = ring_thresholds(n_lines);
        for (int ri = 0; ri < 5; ri++) {
            const float x = rhos[ri] * 0.8f, y = rhos[ri] * -0.6f;
            const double rho = sqrt((double)(x * x + y * y));
            const double g = (double)kRingGuardDeg * LO_PI / 180.0;
            // (a) float by float across three guards on either side of every threshold (the guard band and both its edges)
            for (double t : thr) {
                const double c = t * LO_PI / 180.0;
                const float zl = (float)(rho * tan(c - 3.0 * g)), zh = (float)(rho * tan(c + 3.0 * g));
                const float marks[3] = { (float)(rho * tan(c - g)), (float)(rho * tan(c)), (float)(rho * tan(c + g)) };
                sweep_z(x, y, zl, zh, marks, 3, n_lines, thr, 400000, 3000, 20000);            // only a threshold at 0 deg is too dense for every float
            }
            // (b) the whole interval of the polynomial and beyond it (tan 35 deg, where t alone discards), strided
            const float zm = (float)(rho * 0.7);
            const float marks[2] = { -0.0f, 0.0f };
            sweep_z(x, y, -zm, zm, marks, 2, n_lines, thr, 0, 3000, 200000);
            // (c) far outside: up to the largest finite z
            const float big[6] = { (float)(rho * 5.0), 1e6f, 1e20f, 3.4e38f, 1e-30f, 1e-42f };
            for (int b = 0; b < 6; b++) { check_ring(x, y, big[b], n_lines, thr); check_ring(x, y, -big[b], n_lines, thr); }
        }
    }
}

static void check_half(float x, float y, float x0, float y0)
{
    const float startOri = (float)(-lo_atan2((double)y0, (double)x0));
    float ux, uy;
    ring_start_dir(x0, y0, ux, uy);
    const bool want = exact_half(x, y, startOri);
    // true wrapped difference of the two azimuths, in [-pi / 2, 3 pi / 2)
    double d = -lo_atan2((double)y, (double)x) + lo_atan2((double)y0, (double)x0);
    while (d < -LO_PI / 2.0) d += 2.0 * LO_PI;
    while (d >= 1.5 * LO_PI) d -= 2.0 * LO_PI;
    const double dist = fmin(fabs(d - LO_PI), fmin(fabs(d + LO_PI / 2.0), fabs(d - 1.5 * LO_PI)));
    const bool far = dist > 2.0 * (double)kHalfGuardRad;
    const float q2 = x * x + y * y;
    const float rs0 = (float)(1.0 / sqrt((double)q2));
    const float rsv[3] = { rs0, nextafterf(rs0, 0.0f), nextafterf(rs0, INFINITY) };
    for (int v = 0; v < 3; v++) {
        bool past;
        n_checked++;
        const bool decided = half_fast(x, y, q2 * rsv[v], ux, uy, past);
        if (decided) n_fast++; else n_fallback++;
        const bool wrong = decided && past != want, ff = !decided && far;
        n_wrong += wrong; n_far_fallback += ff;
        if ((wrong || ff) && n_printed++ < 20)
            std::printf("half x=%.9g y=%.9g start=(%.9g, %.9g) d=%.12g: %s fast=%d exact=%d\n", x, y, x0, y0, d, wrong ? "WRONG" : "FAR FALLBACK", (int)past, (int)want);
    }
}

static void azimuth_sweeps()
{
    // start directions: the four axes (with both signs of zero), one per quadrant, two near an axis, x0 = y0 = 0
    const float starts[13][2] = { { 7.0f, 0.0f }, { 7.0f, -0.0f }, { 0.0f, 3.0f }, { -12.0f, 0.0f }, { -12.0f, -0.0f }, { 0.0f, -55.0f }, { 4.1f, 9.3f }, { -8.7f, 2.2f },
                                  { -3.3f, -6.1f }, { 21.0f, -17.5f }, { 30.0f, 1e-4f }, { -1e-5f, -2.5f }, { 0.0f, 0.0f } };
    const float rhos[4] = { 0.6f, 5.3f, 47.0f, 200.0f };
    for (int si = 0; si < 13; si++) {
        const float x0 = starts[si][0], y0 = starts[si][1];
        const double phi0 = -lo_atan2((double)y0, (double)x0);             // angle of (x0, -y0)
        for (int ri = 0; ri < 4; ri++) {
            const double rho = rhos[ri];
            // the two thresholds (pi, 3 pi / 2) and the two quadrant borders that are none (0, pi / 2)
            for (int q = 0; q < 4; q++) {
                const double g = (double)kHalfGuardRad;
                const double dl[4] = { LO_PI, 1.5 * LO_PI, 0.0, 0.5 * LO_PI };
                // across three guards on either side by stepping the coordinate that moves the angle: the smaller one in magnitude
                const double pc = phi0 + dl[q];
                const double xc = rho * cos(pc), yc = -rho * sin(pc);
                const bool step_y = fabs(yc) <= fabs(xc);
                double lo = 1e300, hi = -1e300, mk[3];
                for (int e = -3; e <= 3; e++) {
                    const double p = pc + e * g, c = step_y ? -rho * sin(p) : rho * cos(p);
                    lo = fmin(lo, c); hi = fmax(hi, c);
                    if (e >= -1 && e <= 1) mk[e + 1] = c;
                }
                const float marks[5] = { (float)mk[0], (float)mk[1], (float)mk[2], 0.0f, -0.0f };
                const int64_t k0 = fkey((float)lo), k1 = fkey((float)hi);
                const float fx = (float)xc, fy = (float)yc;
                if (k1 - k0 <= 400000) {
                    for (int64_t k = k0; k <= k1; k++) step_y ? check_half(fx, fval(k), x0, y0) : check_half(fval(k), fy, x0, y0);
                } else {                                                        // the stepped coordinate passes through 0: every float near the marks, a stride between
                    for (int m = 0; m < 5; m++) {
                        const int64_t c = fkey(marks[m]);
                        if (c < k0 - 3000 || c > k1 + 3000) continue;
                        for (int64_t k = c - 3000; k <= c + 3000; k++) step_y ? check_half(fx, fval(k), x0, y0) : check_half(fval(k), fy, x0, y0);
                    }
                    const int64_t step = (k1 - k0) / 20000 + 1;
                    for (int64_t k = k0; k <= k1; k += step) step_y ? check_half(fx, fval(k), x0, y0) : check_half(fval(k), fy, x0, y0);
                }
            }
            // the whole circle
            for (int k = 0; k < 20000; k++) {
                const double p = 2.0 * LO_PI * (k + 0.37) / 20000.0;
                check_half((float)(rho * cos(p)), (float)(-rho * sin(p)), x0, y0);
            }
        }
    }
}

int main()
{
    elevation_sweeps();
    const long long ring_checked = n_checked, ring_fast_n = n_fast, ring_fb = n_fallback;
    azimuth_sweeps();
    // inputs the fast path must hand over whole: x = y = 0, x x + y y outside [1e-30, 1e30]
    int id; bool past; int handed = 0;
    handed += fast_decide(0.0f, 0.0f, 1.0f, 64, 1.0f, 0.0f, 1.0f, id, past) == 0;
    handed += fast_decide(-0.0f, 0.0f, -1.0f, 16, 1.0f, 0.0f, 1.0f, id, past) == 0;
    handed += fast_decide(1e-16f, 1e-17f, 0.6f, 32, 1.0f, 0.0f, 1e16f, id, past) == 0;
    handed += fast_decide(2e15f, 1.0f, 0.6f, 64, 1.0f, 0.0f, 5e-16f, id, past) == 0;
    handed += fast_decide(3e38f, 3e38f, 0.6f, 64, 1.0f, 0.0f, 0.0f, id, past) == 0;
    std::printf("ring: checked=%lld fast=%lld fallback=%lld | half: checked=%lld fast=%lld fallback=%lld | handed_over=%d/5 | wrong=%lld far_fallback=%lld\n",
                ring_checked, ring_fast_n, ring_fb, n_checked - ring_checked, n_fast - ring_fast_n, n_fallback - ring_fb, handed, n_wrong, n_far_fallback);
    return (n_wrong || n_far_fallback || handed != 5) ? 1 : 0;
}
