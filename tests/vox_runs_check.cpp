// Host check of lmono_amd/csrc/vox_runs.hpp: vox_run_length (a window of two bitmap words and a count of trailing ones) against the
// walk it replaced, one bit after the other:   rl = 1; while (i0 + rl < len && bit(i0 + rl)) rl++;
//
// The bitmap is k_voxel's: bit i = "point i continues the run of point i - 1", the head's own bit is 0, no bit at or behind len is set,
// and two zero words follow the words of the ring.
//   1. every head position i0 and every run length that fits, over a ring of three words (len = 192) and of len = 150, 129, 128, 127,
//      65, 64, 63: one run in an otherwise empty bitmap, and the same run with every other bit of the ring set as well
//      (neighbouring runs on both sides, separated from it by the head's own zero bit and the zero behind the run);
//   2. the runs that end at bits 63, 64 and 127 and at the last point of the ring, from every head (part of 1, counted separately);
//   3. bitmaps whose words are all ones (one run from point 0 over one, two and three whole words) and all zeros (every run has length 1);
//   4. 20 000 random bitmaps of random density over up to 36 words (2304 points, the small instantiation's ring), every head checked.
// Prints "checked=<n> ends63=<n> ends64=<n> ends127=<n> endslen=<n> wrong=<n>" as its last line; exit status 1 when wrong != 0.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../lmono_amd/csrc/vox_runs.hpp"

static int walk(const std::vector<unsigned long long> &w, int i0, int len)
{
    int rl = 1;
    while (i0 + rl < len && ((w[(i0 + rl) >> 6] >> ((i0 + rl) & 63)) & 1ull)) rl++;
    return rl;
}

static long long checked = 0, wrong = 0, ends63 = 0, ends64 = 0, ends127 = 0, endslen = 0;

static void check(const std::vector<unsigned long long> &w, int i0, int len)
{
    const int a = vox_run_length(w.data(), i0), b = walk(w, i0, len);
    checked++;
    if (a != b) { if (wrong < 10) printf("wrong: i0=%d len=%d helper=%d walk=%d\n", i0, len, a, b); wrong++; }
    const int last = i0 + b - 1;
    if (last == 63) ends63++;
    if (last == 64) ends64++;
    if (last == 127) ends127++;
    if (last == len - 1) endslen++;
}

static void set_bit(std::vector<unsigned long long> &w, int i) { w[i >> 6] |= 1ull << (i & 63); }
static void clr_bit(std::vector<unsigned long long> &w, int i) { w[i >> 6] &= ~(1ull << (i & 63)); }

int main()
{
    // 1, 2: every head and run length
    const int lens[] = {192, 150, 129, 128, 127, 65, 64, 63};
    for (int len : lens) {
        const int words = (len + 63) / 64;
        for (int crowded = 0; crowded < 2; crowded++)
            for (int i0 = 0; i0 < len; i0++)
                for (int rl = 1; i0 + rl <= len; rl++) {
                    std::vector<unsigned long long> w(words + 2, 0ull);
                    if (crowded) for (int i = 1; i < len; i++) set_bit(w, i);
                    clr_bit(w, i0);
                    for (int i = i0 + 1; i < i0 + rl; i++) set_bit(w, i);
                    if (i0 + rl < len) clr_bit(w, i0 + rl);
                    check(w, i0, len);
                    if (crowded && i0 + rl < len) check(w, i0 + rl, len);      // the neighbouring run behind it
                }
    }
    // 3: whole words of ones and of zeros
    for (int full = 1; full <= 3; full++) {
        const int len = 64 * full;
        std::vector<unsigned long long> w(full + 2, 0ull);
        for (int k = 0; k < full; k++) w[k] = ~0ull;
        clr_bit(w, 0);                      // point 0 is the head
        check(w, 0, len);
        std::vector<unsigned long long> w2(full + 3, 0ull);          // the same behind a word of zeros: the head is the last bit of word 0
        for (int k = 1; k <= full; k++) w2[k] = ~0ull;
        check(w2, 63, 64 + len);
        std::vector<unsigned long long> z(full + 2, 0ull);
        for (int i0 = 0; i0 < len; i0++) check(z, i0, len);
    }
    // 4: random bitmaps
    uint64_t s = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int it = 0; it < 20000; it++) {
        const int len = 12 + (int)(rnd() % 2293);                     // 12 .. 2304
        const int words = (len + 63) / 64;
        const unsigned int dens = (unsigned int)(rnd() % 257);       // ones per 256: 0 = empty .. 256 = full
        std::vector<unsigned long long> w(words + 2, 0ull);
        for (int i = 1; i < len - 6; i++) if ((rnd() & 255) < dens) set_bit(w, i);
        for (int i0 = 0; i0 < len; i0++)
            if (!((w[i0 >> 6] >> (i0 & 63)) & 1ull)) check(w, i0, len);
    }
    printf("checked=%lld ends63=%lld ends64=%lld ends127=%lld endslen=%lld wrong=%lld\n", checked, ends63, ends64, ends127, endslen, wrong);
    return wrong ? 1 : 0;
}
