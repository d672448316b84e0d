// Host check of lmono_amd/csrc/sel_rounds.hpp: the sharp picks of a sector settled in parallel rounds, the header's own predicates
// run lane by lane as k_select runs them (blocked layout, M = 5 / 6 / 11 elements a lane, halo of five from the lanes next door,
// members ranked by key, the first 20 taken; more than 64 members: those below the 20th largest lane maximum left out, and the
// sequential arg-max loop with the header's hit mask if more than 64 remain), against
// the reference walk: sort by (curvature, index), take the next unsuppressed, mark its reach, stop at 20.
//
// A sector here is a stretch of a ring with kPad points of the neighbouring sectors on either side (marks land there).  key[e] is the
// curvature word of element e, 0 for a point that is no candidate (c <= 0.1); flag[i] is the gap flag between ring points i and i + 1.
// Compared: the picks in order, their number, and every picked byte of the ring afterwards.
//
// Last line: checked=<sectors> ties=<..> staircases=<..> fallback=<..> filtered=<..> over20=<..> edge=<..> maxrounds=<..> wrong=<..>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <thread>
#include <vector>

#include "../lmono_amd/csrc/sel_rounds.hpp"

namespace {

constexpr int kPad = 8, kMaxLen = 704, kRing = kMaxLen + 2 * kPad;

struct Sector {
    int slen = 0;
    unsigned int key[kMaxLen];
    unsigned char flag[kRing + 8];
    unsigned char picked0[kRing];      // marks of the sector before
};

struct Result {
    int n = 0, rounds = 0, members = 0;
    bool fallback = false;
    int pick[kSelSharpMax];
    unsigned char picked[kRing];
    bool same(const Result &o, int rlen) const { return n == o.n && std::equal(pick, pick + n, o.pick) && std::memcmp(picked, o.picked, rlen) == 0; }
};

inline int reach_f(const Sector &s, int i) { int l = 0; while (l < kSelReach && !s.flag[i + l]) l++; return l; }
inline int reach_b(const Sector &s, int i) { int l = 0; while (l < kSelReach && !s.flag[i - 1 - l]) l++; return l; }

void reference(const Sector &s, Result &r)
{
    std::memcpy(r.picked, s.picked0, s.slen + 2 * kPad);
    static thread_local std::vector<std::pair<unsigned long long, int>> order;
    order.clear();
    for (int e = 0; e < s.slen; e++)
        if (s.key[e]) order.push_back({((unsigned long long)s.key[e] << 32) | (unsigned int)(kPad + e), kPad + e});
    std::sort(order.begin(), order.end());
    r.n = 0;
    for (int k = (int)order.size() - 1; k >= 0; k--) {
        const int i = order[k].second;
        if (r.picked[i]) continue;
        r.pick[r.n++] = i;
        const int lf = reach_f(s, i), lb = reach_b(s, i);
        for (int q = i - lb; q <= i + lf; q++) r.picked[q] = 1;
        if (r.n >= kSelSharpMax) break;
    }
}

// the kernel's sector, lane by lane
template <int M>
void rounds(const Sector &s, Result &r, int &dead_mismatch)
{
    const int nl = std::min(64, (s.slen + M - 1) / M + 1);       // lanes behind the sector's end hold nothing: one of them is kept
    static thread_local unsigned int kh[64][M], kl[64][M], live[64], dead[64], big[64], mem[64], win[64];
    std::memcpy(r.picked, s.picked0, s.slen + 2 * kPad);
    static thread_local unsigned int gaps[64];
    for (int L = 0; L < nl; L++) {
        // the lane's gap window as the kernel reads it: 32 flags from five positions before the lane's first element (flags behind the
        // ring's words read as 0); a lane that holds no element reads nothing
        gaps[L] = 0u;
        if (L * M < s.slen)
            for (int q = 0; q < 32; q++) {
                const int fi = kPad + L * M - kSelReach + q;
                if (fi < s.slen + 2 * kPad + 8 && s.flag[fi]) gaps[L] |= 1u << q;
            }
        live[L] = dead[L] = big[L] = mem[L] = 0u;
        for (int m = 0; m < M; m++) {
            const int e = L * M + m;
            kh[L][m] = kl[L][m] = 0u;
            if (e < s.slen) {
                const int i = kPad + e;
                kh[L][m] = s.key[e];
                kl[L][m] = ((unsigned int)i << 8) | (unsigned int)reach_f(s, i) | ((unsigned int)reach_b(s, i) << 4);
                if (s.picked0[i]) dead[L] |= 1u << m;
                if (s.key[e]) big[L] |= 1u << m;
            } else dead[L] |= 1u << m;
        }
        live[L] = big[L] & ~dead[L];
    }
    r.rounds = 0;
    while (true) {
        bool any = false;
        for (int L = 0; L < nl; L++) any |= live[L] != 0u;
        if (!any) break;
        r.rounds++;
        for (int L = 0; L < nl; L++) {
            unsigned int x[M + 2 * kSelReach];
            for (int p = -kSelReach; p < M + kSelReach; p++) {
                int LL = L, m = p;
                if (p < 0) { LL = L - 1; m = p + M; }
                if (p >= M) { LL = L + 1; m = p - M; }
                x[p + kSelReach] = (LL >= 0 && LL < nl && ((live[LL] >> m) & 1u)) ? kh[LL][m] : 0u;
            }
            win[L] = sel_winners<M>(x, gaps[L]);
        }
        for (int L = 0; L < nl; L++) {
            mem[L] |= win[L];
            const unsigned int w = sel_window<M>(L > 0 ? win[L - 1] : 0u, win[L], L + 1 < nl ? win[L + 1] : 0u);
            live[L] &= ~sel_deaths<M>(w, gaps[L]);
        }
    }
    // members one per lane, ranked by key
    static thread_local std::vector<std::pair<unsigned int, unsigned int>> c;
    c.clear();
    r.members = 0;
    for (int L = 0; L < nl; L++) r.members += __builtin_popcount(mem[L]);
    static thread_local unsigned int top[64];
    for (int L = 0; L < nl; L++) top[L] = mem[L];
    if (r.members > 64) {
        // the members below the 20th largest of the lanes' best curvatures are left out of the ranking (all 64 lanes of the wave take part)
        unsigned int best[64], bound = ~0u;
        for (int L = 0; L < 64; L++) best[L] = L < nl ? sel_lane_best<M>(mem[L], kh[L]) : 0u;
        for (int L = 0; L < 64; L++) {
            int above = 0;
            for (int t = 0; t < 64; t++) above += best[t] > best[L] ? 1 : 0;
            if (above < kSelSharpMax && best[L] < bound) bound = best[L];
        }
        for (int L = 0; L < nl; L++) top[L] = sel_keep_from<M>(mem[L], kh[L], bound);
    }
    for (int m = 0; m < M; m++)
        for (int L = 0; L < nl; L++)
            if ((top[L] >> m) & 1u) c.push_back({kh[L][m], kl[L][m]});
    r.n = 0;
    r.fallback = c.size() > 64;
    if (!r.fallback) {
        for (size_t a = 0; a < c.size(); a++) {
            int rank = 0;
            for (size_t t = 0; t < c.size(); t++) rank += sel_key_above(c[t].first, c[t].second, c[a].first, c[a].second) ? 1 : 0;
            if (rank < kSelSharpMax) {
                const int pind = (int)(c[a].second >> 8), lf = sel_lf(c[a].second), lb = sel_lb(c[a].second);
                r.pick[rank] = pind;
                for (int o = 0; o <= 2 * kSelReach; o++) if (o <= lf + lb) r.picked[pind - lb + o] = 1;
            }
        }
        r.n = std::min(r.members, kSelSharpMax);
    } else {
        // the sequential loop, the slot mask `dead` kept up to date by the header's hit mask
        while (true) {
            unsigned int bh = 0u, bl = 0u;
            for (int L = 0; L < nl; L++)
                for (int m = 0; m < M; m++)
                    if (((big[L] & ~dead[L]) >> m) & 1u)
                        if (sel_key_above(kh[L][m], kl[L][m], bh, bl) || (bh == 0u && bl == 0u)) { bh = kh[L][m]; bl = kl[L][m]; }
            if (bh == 0u) break;
            if (r.n >= kSelSharpMax) break;
            const int pind = (int)(bl >> 8), lf = sel_lf(bl), lb = sel_lb(bl);
            r.pick[r.n++] = pind;
            for (int o = 0; o <= lf + lb; o++) r.picked[pind - lb + o] = 1;
            for (int L = 0; L < nl; L++) dead[L] |= sel_hit_bits<M>(pind - lb - kPad - L * M, lb + lf);
        }
        // the mask the flat picks would start from = the picked bytes of the sector
        for (int L = 0; L < nl; L++)
            for (int m = 0; m < M; m++) {
                const int e = L * M + m;
                const bool want = e >= s.slen || r.picked[kPad + e];
                if ((((dead[L] >> m) & 1u) != 0u) != want) dead_mismatch++;
            }
    }
}

struct Tally {
    long checked = 0, wrong = 0, ties = 0, staircases = 0, fallback = 0, filtered = 0, over20 = 0, edge = 0, hit_wrong = 0;
    int maxrounds = 0;
    void add(const Tally &o)
    {
        checked += o.checked; wrong += o.wrong; ties += o.ties; staircases += o.staircases; fallback += o.fallback; filtered += o.filtered;
        over20 += o.over20; edge += o.edge; hit_wrong += o.hit_wrong; maxrounds = std::max(maxrounds, o.maxrounds);
    }
};

int run(const Sector &s, Tally &t, int force_m = 0)
{
    Result a, b;
    reference(s, a);
    int dm = 0;
    const int M = force_m ? force_m : (s.slen <= 5 * 64 ? 5 : s.slen <= 6 * 64 ? 6 : 11);
    if (M == 5) rounds<5>(s, b, dm); else if (M == 6) rounds<6>(s, b, dm); else rounds<11>(s, b, dm);
    t.checked++;
    if (!a.same(b, s.slen + 2 * kPad)) { if (t.wrong < 5) std::printf("MISMATCH slen=%d M=%d n=%d/%d members=%d\n", s.slen, M, a.n, b.n, b.members); t.wrong++; }
    t.hit_wrong += dm;
    if (b.fallback) t.fallback++;
    if (b.members > 64 && !b.fallback) t.filtered++;
    if (b.members > kSelSharpMax) t.over20++;
    t.maxrounds = std::max(t.maxrounds, b.rounds);
    return b.rounds;
}

void clear(Sector &s, int slen)
{
    s.slen = slen;
    // only the sector's own stretch of the ring is used (the exhaustive sweep makes millions of short sectors)
    std::memset(s.key, 0, sizeof(unsigned int) * slen);
    std::memset(s.flag, 0, slen + 2 * kPad + 8);
    std::memset(s.picked0, 0, slen + 2 * kPad);
}

// every ordering of n keys that starts with key `first` x every mask of the gaps between the keys
void exhaustive(int n, int first, Tally &t)
{
    static thread_local Sector s;
    int rest[8], perm[8];
    for (int k = 0, q = 0; k < n; k++) if (k != first) rest[q++] = k;
    unsigned int pc = 7919u * (unsigned int)first;
    do {
        perm[0] = first;
        for (int k = 1; k < n; k++) perm[k] = rest[k - 1];
        for (unsigned int g = 0; g < (1u << (n - 1)); g++) {
            clear(s, 2 + n + (int)(pc % 3u));
            for (int k = 0; k < n; k++) s.key[2 + k] = 0x3e000000u + 16u * (unsigned int)perm[k];
            for (int k = 0; k + 1 < n; k++) s.flag[kPad + 2 + k] = (g >> k) & 1u;
            const unsigned int h = pc * 2654435761u + g * 40503u;
            s.flag[kPad + 1] = (h >> 7) & 1u; s.flag[kPad] = (h >> 9) & 1u; s.flag[kPad + 2 + n - 1] = (h >> 11) & 1u; s.flag[kPad + 2 + n] = (h >> 13) & 1u;
            run(s, t);
        }
        pc++;
    } while (std::next_permutation(rest, rest + n - 1));
}

}  // namespace

int main(int argc, char **argv)
{
    // "short": the sweep of a sanitized build (the exhaustive part stops at 6 keys; a quarter of the gap masks at the borders and of the
    // random sectors)
    const bool brief = argc > 1 && std::strcmp(argv[1], "short") == 0;
    Tally t;
    static Sector s;
    std::mt19937 rng(12345);

    // 1. every ordering of up to 8 keys x every mask of the gaps between them; the keys straddle a lane boundary (elements 2 ..),
    //    the flags on either side come from the case number.  One thread per first key: the orderings of 8 keys are 5.2 M sectors.
    for (int n = 1; n <= (brief ? 6 : 8); n++) {
        std::vector<Tally> part(n);
        std::vector<std::thread> pool;
        for (int first = 0; first < n; first++) pool.emplace_back(exhaustive, n, first, std::ref(part[first]));
        for (auto &th : pool) th.join();
        for (const Tally &q : part) t.add(q);
    }

    // 2. ties in curvature at distances 1 .. 6, every mask of the gaps between the two, with and without a larger key nearby,
    //    at every offset against the lane boundaries of all three layouts
    for (int M : {5, 6, 11})
        for (int d = 1; d <= 6; d++)
            for (int at = 0; at < 2 * M; at += (brief ? 3 : 1))
                for (unsigned int g = 0; g < (1u << d); g++)
                    for (int extra = 0; extra < 3; extra++) {
                        clear(s, M == 5 ? 320 : M == 6 ? 384 : 704);
                        s.key[at] = s.key[at + d] = 0x3e800000u;
                        for (int k = 0; k < d; k++) s.flag[kPad + at + k] = (g >> k) & 1u;
                        if (extra == 1) s.key[at + d + 2] = 0x3e800000u;
                        if (extra == 2) s.key[at + d + 3] = 0x3f000000u;
                        run(s, t);
                        t.ties++;
                    }

    // 3. monotone staircases, all gaps short: one member per round, ceil(n / 6) rounds
    for (int n = 30; n <= 300; n++)
        for (int up = 0; up < 2; up++) {
            clear(s, n <= 310 ? 320 : 384);
            for (int k = 0; k < n; k++) s.key[3 + k] = 0x3e000000u + 8u * (unsigned int)(up ? k : n - 1 - k);
            const int r = run(s, t);
            if (r != (n + 5) / 6) { std::printf("staircase n=%d up=%d rounds=%d\n", n, up, r); t.wrong++; }
            t.staircases++;
        }

    // 4. all gaps long: every candidate is a member (more than 20, more than 64: the sequential loop), all three layouts
    for (int slen : {40, 64, 65, 130, 320, 321, 384, 385, 704})
        for (int every = 1; every <= 3; every++)
            for (int same = 0; same < 3; same++) {       // distinct curvatures; one curvature (nothing can be left out: the sequential loop); three
                clear(s, slen);
                std::memset(s.flag, 1, slen + 2 * kPad + 8);
                for (int e = 0; e < slen; e += every) s.key[e] = 0x3e000000u + (same == 0 ? (rng() & 0xffffu) : same == 1 ? 7u : rng() % 3u);
                run(s, t);
            }

    // 5. reaches across a lane boundary, elements 63 | 64, and both ends of the sector (marks in the neighbouring sectors)
    for (int M : {5, 6, 11})
        for (int at : {0, 1, 4, 5, 6, 59, 60, 63, 64, 65, 69, 70})
            for (int tail = 0; tail < 2; tail++)
                for (unsigned int g = 0; g < 1024u; g += (brief ? 12u : 3u)) {
                    const int slen = M == 5 ? 300 : M == 6 ? 380 : 700;
                    clear(s, slen);
                    const int p = tail ? slen - 1 - (at % 12) : at;
                    s.key[p] = 0x3f000000u;
                    for (int q = std::max(0, p - 5); q <= std::min(slen - 1, p + 5); q++) if (q != p) s.key[q] = 0x3e000000u + (rng() & 0xffu);
                    for (int k = 0; k < 10; k++) s.flag[kPad + p - 5 + k] = (g >> k) & 1u;
                    run(s, t);
                    t.edge++;
                }

    // 6. random sectors of up to 704 points: candidate density, gap density, ties (few distinct curvatures) and old marks all vary
    for (int it = 0; it < (brief ? 5000 : 20000); it++) {
        const int slen = (it % 4 == 0) ? 1 + (int)(rng() % 704u) : 1 + (int)(rng() % 400u);
        clear(s, slen);
        const unsigned int dens = 1u + rng() % 16u, gapd = rng() % 12u, levels = (it % 3 == 0) ? 4u : 0xffffffu, old = rng() % 4u;
        for (int e = 0; e < slen; e++) if (rng() % 16u < dens) s.key[e] = 0x3e000000u + (rng() % levels);
        for (int i = 0; i < slen + 2 * kPad + 8; i++) s.flag[i] = rng() % 12u < gapd;
        if (old == 0u) for (int i = 0; i < slen + 2 * kPad; i++) s.picked0[i] = rng() % 10u == 0u;
        run(s, t);
        if (it % 5 == 0) run(s, t, 11);        // the widest layout takes every length
    }

    std::printf("checked=%ld ties=%ld staircases=%ld fallback=%ld filtered=%ld over20=%ld edge=%ld maxrounds=%d hitmask_wrong=%ld wrong=%ld\n", t.checked, t.ties, t.staircases,
                t.fallback, t.filtered, t.over20, t.edge, t.maxrounds, t.hit_wrong, t.wrong);
    return (t.wrong || t.hit_wrong) ? 1 : 0;
}
