// Host check of lmono_amd/csrc/wave_sum28.hpp: wave_sum28_scatter, the header's own code, over 64 modelled lanes against the butterfly
// it replaces in k_lm_solve (wave_sum_d of common.hpp, once per slot):   for (o = 32; o > 0; o >>= 1) v += v of lane ^ o;
//
// The model.  The value type is 64 doubles side by side (one per lane) with a lane-wise +, and the lane policy restates what the device
// policy's instructions do: pick = select on the lane's bit, xchg = the partner's value, swap = v_permlane32_swap / v_permlane16_swap
// (lanes with the bit clear get the partner's first operand in their second; lanes with the bit set get the partner's second in their first).
//
// Checked, all 28 slots bit for bit (memcmp of the doubles; lanes 2 i and 2 i + 1 both hold slot i):
//   1. 2000 waves of random doubles of mixed sign and of exponents spread over +-40 binades;
//   2. cancelling inputs: +1e300, -1e300 and 1.0 dealt over the lanes, where another pairing order gives other bits -- every placement
//      of the two big values over 64 x 63 lane pairs with 1.0 elsewhere, in slot (a + b) % 28;
//   3. denormals (sums that stay denormal and sums that leave the range), +-infinity (inf + finite, and inf - inf = NaN in every lane
//      that adds them), and one NaN lane among finite ones;
//   4. teeth: the same sums paired in the REVERSE mask order (1, 2, 4, 8, 16, 32) must differ from the butterfly on the cancelling
//      inputs of 2 -- a check that could not tell the orders apart would pass anything.
// Prints "checked=<n> cancelling=<n> special=<n> reverse_differs=<n> wrong=<n>" as its last line; exit status 1 when wrong != 0 or the
// reverse order never differs.
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <limits>
#include <random>

#include "../lmono_amd/csrc/wave_sum28.hpp"

struct V64 { double l[64]; };
static V64 operator+(const V64 &a, const V64 &b) { V64 r; for (int i = 0; i < 64; i++) r.l[i] = a.l[i] + b.l[i]; return r; }

struct ModelLanes {
    template <int kMask> V64 pick(const V64 &a, const V64 &b) const { V64 r; for (int i = 0; i < 64; i++) r.l[i] = (i & kMask) ? b.l[i] : a.l[i]; return r; }
    template <int kMask> V64 xchg(const V64 &a) const { V64 r; for (int i = 0; i < 64; i++) r.l[i] = a.l[i ^ kMask]; return r; }
    template <int kMask> void swap(V64 &a, V64 &b) const
    {
        const V64 a0 = a, b0 = b;
        for (int i = 0; i < 64; i++) {
            if (i & kMask) a.l[i] = b0.l[i ^ kMask];
            else b.l[i] = a0.l[i ^ kMask];
        }
    }
};

// the butterfly of wave_sum_d for one slot; order = the masks in the order they are applied
static void butterfly(const double *in, double *out, const int *order)
{
    double v[64], w[64];
    memcpy(v, in, sizeof v);
    for (int s = 0; s < 6; s++) {
        const int o = order[s];
        for (int i = 0; i < 64; i++) w[i] = v[i] + v[i ^ o];
        memcpy(v, w, sizeof v);
    }
    memcpy(out, v, sizeof v);
}

static const int kFwd[6] = { 32, 16, 8, 4, 2, 1 }, kRev[6] = { 1, 2, 4, 8, 16, 32 };
static long long checked = 0, wrong = 0, reverse_differs = 0;

// in[slot][lane].  Returns whether the reverse order differs from the butterfly in some slot's bytes.
static bool check(const double (*in)[64], const char *what)
{
    static V64 v[32];
    for (int s = 0; s < 32; s++)
        for (int i = 0; i < 64; i++) v[s].l[i] = s < 28 ? in[s][i] : 0.0;
    lmono::wave_sum28_scatter(ModelLanes(), v);
    bool rev_differs = false;
    for (int s = 0; s < 28; s++) {
        double ref[64], rev[64];
        butterfly(in[s], ref, kFwd);
        butterfly(in[s], rev, kRev);
        for (int h = 0; h < 2; h++) {
            const int lane = 2 * s + h;
            checked++;
            // the butterfly leaves in lane L the sum as lane L adds it; lanes differ only in operand order, which + does not see
            if (memcmp(&v[0].l[lane], &ref[lane], 8) != 0) {
                if (wrong < 10) printf("wrong (%s): slot %d lane %d scatter=%a butterfly=%a\n", what, s, lane, v[0].l[lane], ref[lane]);
                wrong++;
            }
            if (memcmp(&rev[lane], &ref[lane], 8) != 0) rev_differs = true;
        }
    }
    return rev_differs;
}

int main()
{
    static double in[28][64];
    std::mt19937_64 rng(20261021);
    std::uniform_real_distribution<double> uni(-1.0, 1.0);
    std::uniform_int_distribution<int> ex(-40, 40);
    // 1. random doubles
    for (int it = 0; it < 2000; it++) {
        for (int s = 0; s < 28; s++)
            for (int i = 0; i < 64; i++) in[s][i] = std::ldexp(uni(rng), ex(rng));
        check(in, "random");
    }
    // 2. cancelling inputs
    long long cancelling = 0;
    for (int a = 0; a < 64; a++)
        for (int b = 0; b < 64; b++) {
            if (a == b) continue;
            for (int s = 0; s < 28; s++)
                for (int i = 0; i < 64; i++) in[s][i] = uni(rng);
            double *row = in[(a + b) % 28];
            for (int i = 0; i < 64; i++) row[i] = 1.0;
            row[a] = 1e300; row[b] = -1e300;
            if (check(in, "cancelling")) reverse_differs++;
            cancelling++;
        }
    // 3. denormals, infinities, one NaN lane
    long long special = 0;
    const double dmin = std::numeric_limits<double>::denorm_min(), inf = std::numeric_limits<double>::infinity();
    for (int it = 0; it < 200; it++) {
        for (int s = 0; s < 28; s++)
            for (int i = 0; i < 64; i++) {
                double x;
                switch (s % 7) {
                case 0: x = dmin * (double)(rng() % 1000); break;                                   // stays denormal
                case 1: x = std::ldexp(uni(rng), -1022 - (int)(rng() % 8)); break;                  // around the edge of the normal range
                case 2: x = (rng() & 1) ? -dmin * (double)(rng() % 7) : std::ldexp(uni(rng), -1020); break;
                case 3: x = i == (it + s) % 64 ? inf : uni(rng); break;                             // inf + finite
                case 4: x = i == it % 64 ? inf : (i == (it + 1 + s) % 64 ? -inf : uni(rng)); break; // inf - inf
                case 5: x = i == (it * 7 + s) % 64 ? std::numeric_limits<double>::quiet_NaN() : uni(rng); break;   // one NaN lane
                default: x = (rng() % 5 == 0) ? 0.0 * uni(rng) : std::ldexp(uni(rng), ex(rng)); break;  // signed zeros among ordinary values
                }
                in[s][i] = x;
            }
        check(in, "special");
        special++;
    }
    printf("checked=%lld cancelling=%lld special=%lld reverse_differs=%lld wrong=%lld\n", checked, cancelling, special, reverse_differs, wrong);
    return (wrong != 0 || reverse_differs == 0) ? 1 : 0;
}
