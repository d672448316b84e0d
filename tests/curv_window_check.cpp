// Host check of lmono_amd/csrc/curv_window.hpp: the header over 64 modelled lanes, M = 5, 6, 11 points a lane, against the plain
// per-point loop of k_curvature's expressions, bit for bit (tests/test_curv_window_cpu.py builds and runs this, also under
// -fsanitize=address,undefined).
//
// A sector is the points sp .. sp + slen - 1 of a ring; the lanes load what k_select's select_sector loads (own points clamped to
// ep + 5, lane 0 the five points before the sector, the other lanes what stands behind lane 63).  Compared: the curvature of every
// element, and of every element's window of gap flags the ten bits that k_select reads (points i - 5 .. i + 4).
//
// Swept: random rings; coordinates whose partial sums round differently in another order (and the reverse order of summation is
// counted to differ there, so the comparison can fail); steps whose squared length stands next to 0.05; denormals; sector lengths
// 1, 5, 6, 63 M, 64 M - 1, 64 M and a few between; the sector at the ring's start and at its end (the halo is the ring's first and last
// five points) and inside it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

struct VF { float v[64]; };
struct VU { unsigned int v[64]; };
#define VF_OP(op) static inline VF operator op(const VF &a, const VF &b) { VF r; for (int l = 0; l < 64; l++) r.v[l] = a.v[l] op b.v[l]; return r; }
VF_OP(+) VF_OP(-) VF_OP(*)
static inline VF operator*(int k, const VF &a) { VF r; for (int l = 0; l < 64; l++) r.v[l] = k * a.v[l]; return r; }
static inline VU operator|(const VU &a, const VU &b) { VU r; for (int l = 0; l < 64; l++) r.v[l] = a.v[l] | b.v[l]; return r; }
static inline VU operator<<(const VU &a, int k) { VU r; for (int l = 0; l < 64; l++) r.v[l] = a.v[l] << k; return r; }
static inline VU operator>>(const VU &a, int k) { VU r; for (int l = 0; l < 64; l++) r.v[l] = a.v[l] >> k; return r; }

#include "../lmono_amd/csrc/curv_window.hpp"

static inline VU curv_gap_flag(const VF &gx, const VF &gy, const VF &gz)
{
    VU r;
    for (int l = 0; l < 64; l++) r.v[l] = lmono::curv_gap_flag(gx.v[l], gy.v[l], gz.v[l]);
    return r;
}

struct HostLanes {
    typedef VU bits;
    template <class V> V before(const V &v, const V &old) const { V r; r.v[0] = old.v[0]; for (int l = 1; l < 64; l++) r.v[l] = v.v[l - 1]; return r; }
    template <class V> V behind(const V &v, const V &old) const { V r; r.v[63] = old.v[63]; for (int l = 0; l < 63; l++) r.v[l] = v.v[l + 1]; return r; }
};

struct Ring { std::vector<float> c[3]; int len() const { return (int)c[0].size(); } };

static uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// k_curvature's expressions for point i of a cloud
static float ref_curv(const Ring &r, int i, bool reversed)
{
    float d[3];
    for (int k = 0; k < 3; k++) {
        const float *s = r.c[k].data() + i;
        if (!reversed) d[k] = s[-5] + s[-4] + s[-3] + s[-2] + s[-1] - 10 * s[0] + s[1] + s[2] + s[3] + s[4] + s[5];
        else d[k] = s[5] + s[4] + s[3] + s[2] + s[1] - 10 * s[0] + s[-1] + s[-2] + s[-3] + s[-4] + s[-5];
    }
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
}
static unsigned int ref_gap(const Ring &r, int i)
{
    const float gx = r.c[0][i + 1] - r.c[0][i], gy = r.c[1][i + 1] - r.c[1][i], gz = r.c[2][i + 1] - r.c[2][i];
    return ((double)(gx * gx + gy * gy + gz * gz) > 0.05) ? 1 : 0;
}

static long checked = 0, wrong = 0, reverse_differs = 0, gap_set = 0, gap_clear = 0;

template <int M>
static void run_sector(const Ring &r, int sp, int slen)
{
    const int last = slen + 4;
    if (sp < 5 || slen < 1 || slen > 64 * M || sp + last >= r.len()) { std::printf("bad case sp=%d slen=%d len=%d\n", sp, slen, r.len()); wrong++; return; }
    HostLanes lanes;
    VF o[3][M], h[3][lmono::kCurvReach + 1];
    for (int c = 0; c < 3; c++)
        for (int l = 0; l < 64; l++) {
            for (int m = 0; m < M; m++) o[c][m].v[l] = r.c[c][sp + std::min(l * M + m, last)];
            const int hp = sp + (l == 0 ? -lmono::kCurvReach : std::min(64 * M, last));
            const int hmax = l == 0 ? lmono::kCurvReach : std::max(last - 64 * M, 0);
            for (int d = 0; d <= lmono::kCurvReach; d++) h[c][d].v[l] = r.c[c][hp + std::min(d, hmax)];
        }
    const VU hb = lmono::curv_halo_flags<VU>(h[0], h[1], h[2]);
    const VU gwin = lmono::curv_gap_window<M>(lanes, o[0], o[1], o[2], h[0][0], h[1][0], h[2][0], hb);
    VF cv[M];
    for (int c = 0; c < 3; c++) {
        VF hc[lmono::kCurvReach];
        for (int d = 0; d < lmono::kCurvReach; d++) hc[d] = h[c][d];
        lmono::curv_window_coord<M>(lanes, o[c], hc, c == 0, cv);
    }
    for (int e = 0; e < slen; e++) {
        const int l = e / M, m = e % M, i = sp + e;
        const float want = ref_curv(r, i, false);
        checked++;
        if (bits_of(cv[m].v[l]) != bits_of(want)) {
            if (wrong++ < 10) std::printf("M=%d sp=%d slen=%d element %d: curvature %a, expected %a\n", M, sp, slen, e, cv[m].v[l], want);
        }
        if (bits_of(ref_curv(r, i, true)) != bits_of(want)) reverse_differs++;
        for (int k = 0; k < 10; k++) {
            const unsigned int got = (gwin.v[l] >> (m + k)) & 1u, exp = ref_gap(r, i - 5 + k);
            checked++;
            (exp ? gap_set : gap_clear)++;
            if (got != exp && wrong++ < 10) std::printf("M=%d sp=%d slen=%d element %d: gap flag of point %d is %u, expected %u\n", M, sp, slen, e, i - 5 + k, got, exp);
        }
    }
}

enum Kind { kRandom, kCancelling, kThreshold, kDenormal };

static Ring make_ring(std::mt19937 &rng, int len, Kind kind)
{
    Ring r;
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    for (int k = 0; k < 3; k++) r.c[k].resize(len);
    const float step = std::sqrt(0.05f);
    float walk = 0.f;
    for (int i = 0; i < len; i++) {
        const float a = 6.2831853f * i / len;
        switch (kind) {
        case kRandom: {
            const float rho = 20.f + 15.f * u(rng) * (u(rng) > 0.7f ? 1.f : 0.01f);
            r.c[0][i] = rho * std::cos(a); r.c[1][i] = rho * std::sin(a); r.c[2][i] = 0.1f * rho * u(rng);
            break;
        }
        case kCancelling: {
            // large values of either sign between small ones: a partial sum absorbs the small ones or not, depending on the order
            const int t = (int)(rng() % 6);
            for (int k = 0; k < 3; k++)
                r.c[k][i] = t == 0 ? 1.0e8f : t == 1 ? -1.0e8f : t == 2 ? 3.0e7f * u(rng) : u(rng);
            break;
        }
        case kThreshold: {
            // steps along x whose squared length is 0.05 up to a few ulps either way
            walk += std::nextafter(step, u(rng) > 0.f ? 1.f : 0.f) + (float)((int)(rng() % 5) - 2) * 1.5e-8f;
            r.c[0][i] = walk; r.c[1][i] = 0.f; r.c[2][i] = 0.f;
            break;
        }
        case kDenormal:
            for (int k = 0; k < 3; k++) r.c[k][i] = (float)((int)(rng() % 2001) - 1000) * 1.0e-42f;
            break;
        }
    }
    return r;
}

template <int M>
static void sweep(std::mt19937 &rng, Kind kind, long &sectors)
{
    const int lens[] = { 1, 2, 5, 6, M, M + 1, 2 * M + 3, 31 * M + 2, 63 * M, 63 * M + 1, 64 * M - 1, 64 * M };
    for (int slen : lens) {
        // the sector at the ring's start and end at once (both halos are the ring's outermost five points), and inside a longer ring
        const Ring tight = make_ring(rng, slen + 10, kind);
        run_sector<M>(tight, 5, slen);
        const Ring loose = make_ring(rng, slen + 10 + 23, kind);
        run_sector<M>(loose, 5, slen);
        run_sector<M>(loose, 12, slen);
        run_sector<M>(loose, 5 + 23, slen);
        sectors += 4;
    }
}

int main()
{
    std::mt19937 rng(20240611);
    long sectors = 0, cancelling = 0, denormal = 0;
    for (int rep = 0; rep < 3; rep++) {
        sweep<5>(rng, kRandom, sectors); sweep<6>(rng, kRandom, sectors); sweep<11>(rng, kRandom, sectors);
        sweep<5>(rng, kThreshold, sectors); sweep<6>(rng, kThreshold, sectors); sweep<11>(rng, kThreshold, sectors);
    }
    const long set_before = gap_set, clear_before = gap_clear;
    (void)set_before; (void)clear_before;
    reverse_differs = 0;       // counted on the cancelling inputs alone
    {
        const long c0 = checked;
        sweep<5>(rng, kCancelling, sectors); sweep<6>(rng, kCancelling, sectors); sweep<11>(rng, kCancelling, sectors);
        cancelling = checked - c0;
    }
    const long rd = reverse_differs;
    {
        const long c0 = checked;
        sweep<5>(rng, kDenormal, sectors); sweep<6>(rng, kDenormal, sectors); sweep<11>(rng, kDenormal, sectors);
        denormal = checked - c0;
    }
    std::printf("gap flags set=%ld clear=%ld\n", gap_set, gap_clear);
    std::printf("checked=%ld sectors=%ld cancelling=%ld denormal=%ld reverse_differs=%ld wrong=%ld\n", checked, sectors, cancelling, denormal, rd, wrong);
    return wrong == 0 && gap_set > 1000 && gap_clear > 1000 ? 0 : 1;
}
