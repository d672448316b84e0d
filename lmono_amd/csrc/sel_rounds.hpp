// The sharp picks of a sector in parallel rounds, host and device (tests/sel_rounds_check.cpp builds this header with g++).
//
// The reference sorts a sector by (curvature, index), walks the order downwards, takes the next point that no earlier pick
// suppressed, marks the pick's reach [p - lb, p + lf] as suppressed and stops after 20 picks.  lf / lb count the short gaps
// that follow / precede p, five at most.
//
// Why rounds give the same picks:
//  - The reach is symmetric.  q lies in p's reach iff |p - q| <= 5 and every gap flag between the two is clear, which is the
//    same condition read from q.  So "suppresses" is a symmetric conflict relation between candidates.
//  - The greedy walk in descending key order over a symmetric conflict relation yields the lexicographically first maximal
//    independent set, and whether a candidate is a member depends on the candidates of higher key alone.
//  - That set is also what these rounds leave: a live candidate that beats every live candidate within its own reach is a
//    member (nothing of a higher key is left to suppress it), every live candidate within a member's reach dies (by symmetry
//    it tests its own reach for a winner), repeat while anything is live.  Every round settles the largest live key at least.
//  - The walk stops after 20 picks without having looked further, so its picks are the 20 members of highest key, in key
//    order, and only they leave marks.
//
// Layout of a round: lane L of the wave owns the M consecutive elements L*M .. L*M + M - 1 of the sector, so an element's ten
// neighbours are registers of its own lane or of the two lanes next to it.  Position p of a lane is its element p; p = -5 .. -1
// are the last five of the lane before, p = M .. M + 4 the first five of the lane behind.  A round sees
//   x[p + 5]          the live curvature word at position p (0 = not live; a live curvature is > 0.1, so never 0; 0 where the wave ends)
//   gaps, bit p + 5   the gap flag between positions p and p + 1 (the lane's window of the ring's gap bit mask)
// M >= 5.
//
// The key is (curvature bits, index).  A forward neighbour has the larger index and wins a tie in curvature, a backward
// neighbour loses it: ">=" forwards, ">" backwards, and no index is exchanged.
//
// The largest live key within the forward reach of position i is a segmented running maximum, five steps of
//   F_d[i] = gap(i) ? 0 : max(x[i + 1], F_(d-1)[i + 1]),   F_0 = 0
// (backwards the mirror image), so no reach is compared against a distance: a step is one AND and one MAX.  Whether a winner lies
// within reach is the same recurrence over single bits, run on the whole window of a lane at once.
#pragma once

#if defined(__HIPCC__)
#define LMONO_SEL_HD __host__ __device__ __forceinline__
#define LMONO_SEL_UNROLL _Pragma("unroll")
#else
#define LMONO_SEL_HD inline
#define LMONO_SEL_UNROLL
#endif

constexpr int kSelReach = 5;       // the neighbour walk's length
constexpr int kSelSharpMax = 20;   // picks of the sharp phase per sector (the first two are "sharp", all are "less sharp")

// the reach rides in the low byte of an element's low key word: lf | lb << 4
LMONO_SEL_HD int sel_lf(unsigned int kl) { return (int)(kl & 15u); }
LMONO_SEL_HD int sel_lb(unsigned int kl) { return (int)((kl >> 4) & 15u); }

// all ones iff bit q of w is set
LMONO_SEL_HD unsigned int sel_bit_mask(unsigned int w, int q) { return (unsigned int)((int)(w << (31 - q)) >> 31); }
LMONO_SEL_HD unsigned int sel_max(unsigned int a, unsigned int b) { return a > b ? a : b; }

// a live element wins iff no live element of its reach has a larger key
LMONO_SEL_HD bool sel_wins(unsigned int k, unsigned int fwd_max, unsigned int bwd_max) { return k != 0u && fwd_max < k && bwd_max <= k; }

// winners of the lane's M elements as a bit mask (bit m: element m)
template <int M>
LMONO_SEL_HD unsigned int sel_winners(const unsigned int (&x)[M + 2 * kSelReach], unsigned int gaps)
{
    const unsigned int open = ~gaps;             // bit p + 5: positions p and p + 1 see each other
    // step d of the forward maximum lives at positions 5 - d .. 5 - d + M - 1 and reads step d - 1 one position further on, which is the
    // same slot t of f[]; backwards the positions are d - 5 .. d - 5 + M - 1, read one position further back
    // (forwards first and settled, then backwards: the two sets of running maxima are never in registers together)
    unsigned int w = 0u;
    {
        unsigned int f[M];
        LMONO_SEL_UNROLL
        for (int t = 0; t < M; t++) f[t] = sel_bit_mask(open, t + 4 + kSelReach) & x[t + 5 + kSelReach];         // F_1 at i = t + 4: gap(i), x[i + 1]
        LMONO_SEL_UNROLL
        for (int d = 2; d <= kSelReach; d++) {
            LMONO_SEL_UNROLL
            for (int t = 0; t < M; t++) {
                const int i = t + kSelReach - d;
                f[t] = sel_bit_mask(open, i + kSelReach) & sel_max(x[i + 1 + kSelReach], f[t]);
            }
        }
        LMONO_SEL_UNROLL
        for (int m = 0; m < M; m++)
            if (sel_wins(x[m + kSelReach], f[m], 0u)) w |= 1u << m;
    }
    {
        unsigned int b[M], wb = 0u;
        LMONO_SEL_UNROLL
        for (int t = 0; t < M; t++) b[t] = sel_bit_mask(open, t - 5 + kSelReach) & x[t - 5 + kSelReach];         // B_1 at i = t - 4: gap(i - 1), x[i - 1]
        LMONO_SEL_UNROLL
        for (int d = 2; d <= kSelReach; d++) {
            LMONO_SEL_UNROLL
            for (int t = 0; t < M; t++) {
                const int j = t - kSelReach + d;
                b[t] = sel_bit_mask(open, j - 1 + kSelReach) & sel_max(x[j - 1 + kSelReach], b[t]);
            }
        }
        LMONO_SEL_UNROLL
        for (int m = 0; m < M; m++)
            if (sel_wins(x[m + kSelReach], 0u, b[m])) wb |= 1u << m;
        w &= wb;
    }
    return w;
}

// winner bits of the lane and its halo: bit p + 5 = position p (prev / next: the neighbouring lanes' winner masks, 0 where the wave ends)
template <int M>
LMONO_SEL_HD unsigned int sel_window(unsigned int prev, unsigned int own, unsigned int next)
{
    return (prev >> (M - kSelReach)) | (own << kSelReach) | (next << (M + kSelReach));
}

// a live element dies iff a winner lies within its own reach (a winner meets itself there: it leaves the live set as a member): the
// elements of the lane with a winner within reach, from the winners' window
template <int M>
LMONO_SEL_HD unsigned int sel_deaths(unsigned int window, unsigned int gaps)
{
    const unsigned int open = ~gaps, open_b = open << 1;          // bit p + 5: p sees p + 1 / p sees p - 1
    unsigned int r = 0u, s = 0u;
    LMONO_SEL_UNROLL
    for (int d = 1; d <= kSelReach; d++) {
        r = open & ((window | r) >> 1);
        s = open_b & ((window | s) << 1);
    }
    return ((window | r | s) >> kSelReach) & ((1u << M) - 1u);
}

// elements m of the lane with a <= m <= a + span (a: first suppressed element relative to the lane's first, any sign; span <= 10):
// what a pick's reach suppresses in this lane
template <int M>
LMONO_SEL_HD unsigned int sel_hit_bits(int a, int span)
{
    const unsigned int base = (2u << span) - 1u;
    const unsigned int r = a >= 0 ? (a < M ? base << a : 0u) : (a > -16 ? base >> -a : 0u);
    return r & ((1u << M) - 1u);
}

// More members than the 64 that are ranked one per lane: only the 20 of highest key are wanted.  The 20th largest of the lanes' best member
// curvatures is a bound from below on the 20th largest member key (20 members at least reach it), so the members below it can be left out
// before the ranking, and the ranks of the others do not change.
template <int M>
LMONO_SEL_HD unsigned int sel_lane_best(unsigned int members, const unsigned int (&kh)[M])
{
    unsigned int best = 0u;
    LMONO_SEL_UNROLL
    for (int m = 0; m < M; m++) best = sel_max(best, kh[m] & sel_bit_mask(members, m));
    return best;
}
template <int M>
LMONO_SEL_HD unsigned int sel_keep_from(unsigned int members, const unsigned int (&kh)[M], unsigned int bound)
{
    unsigned int keep = 0u;
    LMONO_SEL_UNROLL
    for (int m = 0; m < M; m++) keep |= (unsigned int)(kh[m] >= bound) << m;
    return keep & members;
}

// rank order of two members: (curvature bits, low key word) as one 64-bit key; the low word starts with the index, so no two are equal
LMONO_SEL_HD bool sel_key_above(unsigned int ah, unsigned int al, unsigned int bh, unsigned int bl)
{
    return (((unsigned long long)ah << 32) | al) > (((unsigned long long)bh << 32) | bl);
}
