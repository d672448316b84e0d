// sor.hip -- statistical outlier removal on gfx950: the pcl::StatisticalOutlierRemoval<pcl::PointXYZRGB> that
// MapBuilder::processMapping carries commented out in front of its voxel grid (mono_lidar_mapping/src/map_builder/Map_Builder.cc:24-29),
// as a device-resident filter between the map builder and the voxel map.  The arithmetic is sor.hpp; this file is how the neighbours are found.
//
// One filter call is seven launches for all streams (blockIdx.y = stream), none of which waits on another workgroup.  The first four build the
// grid of the call, without an origin and with the query's work list (cell_grid.hip: clear, cells, offsets, scatter).  Then
//   k_sor_query     the hot kernel.  A workgroup is one wave and takes work items from a counter; an item is up to 64 queries of ONE cell, which share
//                   their neighbourhood.  A query takes a group of 64 / (queries, rounded up to a power of two) adjacent lanes, which deal the
//                   candidates among themselves and add their integer counts and sums with wave shuffles.  For ring r = 1, 2 ... the wave stages
//                   the points of the (2r + 1)^3 cells in LDS tile by tile and each query counts its candidates with d2 <= sor_rho2(r, h).  Queries
//                   that hold k of them are finished at this ring: they find the k-th smallest d2 EXACTLY by a radix select over its bits (non-negative floats order as
//                   uint32; five bits a pass, counting the candidates under the prefix found so far by their next digit, by re-scanning: it
//                   stores counts and no candidate, so it holds for any number of them), then S = sum of u over d2 < tau, plus
//                   (k - count) u(tau).  The ring grows only while a lane of the wave is unfinished.  Per-wave integer reduction of the
//                   statistics, then 64-bit atomic adds.
//   k_sor_flag      every thread forms the threshold from the four words (sor_threshold: identical bits everywhere), writes the keep flag (and
//                   kSorNoScore as the score of a point the grid rejected) and counts a tile's kept points.
//   k_sor_compact   stable compaction into the filter's output cloud: a tile starts where the tiles in front of it end.
#pragma once
#include "common.hpp"
#include "cell_grid.hip"

namespace lmono {

constexpr int kSorT = 256;                // threads of the streaming kernels
constexpr int kSorQ = kCellQ;             // queries of one work item of k_sor_query: one wave
constexpr int kSorTile = 256;             // candidates staged in LDS at a time (4 KB), and as many on their way in registers
constexpr int kSorDigit = 5;              // bits of d2 a pass of the radix select settles (a 32 x 64 histogram in LDS, 8 KB)
constexpr int kSorKeepTile = 1024;        // points per workgroup of k_sor_flag / k_sor_compact

// the 64-bit words of a stream's results; the grid's words (CellWords) lie behind them, from kSorGrid
enum { kSorM = 0, kSorA, kSorBhi, kSorBlo, kSorIsolated, kSorKept, kSorRingSum, kSorSelected, kSorNext, kSorGrid, kSorWords = 16 };
static_assert(8 * kSorGrid + sizeof(CellWords) <= 8 * kSorWords, "the grid's words fit behind the filter's");

struct SorJob {
    CellView g;                            // the call's cloud and its grid; g.w lies in st
    int k;
    double mul;
    unsigned *v;                           // per input point: score, kSorNoScore when rejected or isolated
    unsigned char *keep;
    unsigned *tile_n;                      // kept points per tile of kSorKeepTile
    PtRgb *out;
    unsigned long long *st;                // [kSorWords]
};

// The points of the cells within ring r of cell (cx, cy, cz), staged in LDS tile by tile.  The lanes of a group (`group` lanes, a power of two;
// `sub` = the lane's place in its group) share one query and deal a tile's points among themselves: f(point) runs for every point on
// exactly one lane of each group, and lanes with the same `sub` read the same staged point at the same time (a broadcast).
template <typename F> __device__ inline void sor_scan(const CellView &g, int cx, int cy, int cz, int r, unsigned group, unsigned sub, CellPt *tile, unsigned *seg_pre, unsigned *seg_off, F f)
{
    const int lane = threadIdx.x;
    const int side = 2 * r + 1, cells = side * side * side;
    for (int c0 = 0; c0 < cells; c0 += 64) {
        const int cid = c0 + lane;
        unsigned n = 0, o = 0;
        if (cid < cells) {
            const int x = cx + cid % side - r, y = cy + cid / side % side - r, z = cz + cid / (side * side) - r;
            constexpr int L = 1 << 20;
            if (x >= -L && x < L && y >= -L && y < L && z >= -L && z < L) {
                const unsigned slot = cellgrid_find(g, vm_key(x, y, z));
                if (slot != kCellNoSlot) { n = g.cnt[slot]; o = g.off[slot]; }
            }
        }
        unsigned incl = n;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned y = __shfl_up(incl, d);
            if (lane >= d) incl += y;
        }
        const unsigned total = __shfl(incl, 63);
        __syncthreads();                                   // the segments of the chunk before are no longer read
        seg_pre[lane] = incl - n; seg_off[lane] = o;
        __syncthreads();
        // the points of the tile at t0 into registers: a tile is fetched while the tile before it is scanned
        CellPt buf[kSorTile / 64];
        auto fetch = [&](unsigned t0) {
#pragma unroll
            for (int u = 0; u < kSorTile / 64; u++) {
                const unsigned p = t0 + 64u * u + lane;
                if (p >= total) continue;
                int s = 0;                                  // the last segment that starts at or before p: it is not empty, since p < total
                for (int step = 32; step > 0; step >>= 1) if (seg_pre[s + step] <= p) s += step;
                buf[u] = g.sorted[seg_off[s] + (p - seg_pre[s])];
            }
        };
        if (total) fetch(0);
        for (unsigned t0 = 0; t0 < total; t0 += kSorTile) {
            const unsigned m = total - t0 < (unsigned)kSorTile ? total - t0 : (unsigned)kSorTile;
            __syncthreads();                               // the tile before has been scanned
#pragma unroll
            for (int u = 0; u < kSorTile / 64; u++) if (64u * u + lane < m) tile[64u * u + lane] = buf[u];
            __syncthreads();
            if (t0 + kSorTile < total) fetch(t0 + kSorTile);
#pragma unroll 4
            for (unsigned e = sub; e < m; e += group) f(tile[e]);
        }
    }
}

__device__ inline unsigned long long sor_wave_sum(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the sum of x over the lanes of a group (a power of two of adjacent lanes, the same for the whole wave), on every lane of it
template <typename T> __device__ inline T sor_group_sum(T x, unsigned group)
{
    for (unsigned o = group >> 1; o > 0; o >>= 1) x += __shfl_xor(x, (int)o);
    return x;
}

__global__ __launch_bounds__(kSorQ) void k_sor_query(const SorJob *jobs)
{
    const SorJob &j = jobs[blockIdx.y];
    if (j.g.n == 0) return;
    __shared__ CellPt tile[kSorTile];
    __shared__ unsigned seg_pre[64], seg_off[64];
    __shared__ unsigned hist[1 << kSorDigit][kSorQ];
    const int lane = threadIdx.x;
    const unsigned nwork = j.g.w->nwork;
    const unsigned k = (unsigned)j.k;
    unsigned long long sM = 0, sA = 0, sBhi = 0, sBlo = 0, sIso = 0, sRing = 0;
    for (;;) {
        // items differ in cost by orders of magnitude (a query that ends isolated looks at 17^3 cells at 8 rings): the next one from a counter
        unsigned w = 0;
        if (lane == 0) w = (unsigned)atomicAdd(&j.st[kSorNext], 1ull);
        w = __shfl(w, 0);
        if (w >= nwork) break;
        const CellWork wk = j.g.work[w];
        const unsigned long long key = j.g.key[wk.slot];
        const int cx = (int)(key & 0x1fffff) - (1 << 20), cy = (int)(key >> 21 & 0x1fffff) - (1 << 20), cz = (int)(key >> 42 & 0x1fffff) - (1 << 20);
        // the item's queries (at most 64) take `group` adjacent lanes each: the largest power of two that fits them into the wave.  Most cells of a
        // frame cloud hold far fewer than 64 points; their queries would leave most of the wave idle
        const unsigned nq = min(j.g.cnt[wk.slot] - wk.tile * kSorQ, (unsigned)kSorQ);
        unsigned group = 1, shift = 0;
        while (nq * (group << 1) <= (unsigned)kSorQ) { group <<= 1; shift++; }
        const unsigned sub = lane & (group - 1), qi = wk.tile * kSorQ + (lane >> shift);
        const bool mine = (unsigned)lane >> shift < nq;
        CellPt q = { 0.0f, 0.0f, 0.0f, kCellNoSlot };
        if (mine) q = j.g.sorted[j.g.off[wk.slot] + qi];
        bool active = mine;
        unsigned v = kSorNoScore;
        for (int r = 1; r <= j.g.rings && __any(active); r++) {
            const float bound = sor_rho2(r, j.g.h);
            unsigned c = 0;
            sor_scan(j.g, cx, cy, cz, r, group, sub, tile, seg_pre, seg_off, [&](const CellPt &p) {
                if (p.i != q.i && sor_d2(q.x, q.y, q.z, p.x, p.y, p.z) <= bound) c++;
            });
            c = sor_group_sum(c, group);
            const bool fin = active && c >= k;
            if (active && sub == 0) sRing++;
            if (!__any(fin)) continue;
            // Radix select, kSorDigit bits a pass from the highest bit of `bound` down (the k-th smallest d2 of a finished lane lies at or below
            // `bound`, so a candidate with a higher bit set is above it and is never counted).  A pass counts, per lane, the candidates that share
            // the prefix found so far by their next digit (hist[digit][lane]: a lane touches its own column only); the digit that holds the k-th
            // smallest extends the prefix, and `below` counts the candidates under it.
            unsigned prefix = 0, below = 0;
            for (int hi = 31 - __clz((int)(__float_as_uint(bound) | 1u)); hi >= 0; hi -= kSorDigit) {
                const int lo = hi >= kSorDigit - 1 ? hi - (kSorDigit - 1) : 0;
                const unsigned dmax = (2u << (hi - lo)) - 1u, want = prefix >> (hi + 1);
                for (unsigned d = 0; d <= dmax; d++) hist[d][lane] = 0;
                sor_scan(j.g, cx, cy, cz, r, group, sub, tile, seg_pre, seg_off, [&](const CellPt &p) {
                    const unsigned bits = __float_as_uint(sor_d2(q.x, q.y, q.z, p.x, p.y, p.z));
                    if (p.i != q.i && bits >> (hi + 1) == want) atomicAdd(&hist[bits >> lo & dmax][lane], 1u);      // no-return LDS add: the scan does not wait for it
                });
                unsigned digit = 0;
                bool found = false;
                for (unsigned d = 0; d <= dmax; d++) {
                    const unsigned c = sor_group_sum(hist[d][lane], group);
                    if (!found && below + c >= k) { digit = d; found = true; }
                    if (!found) below += c;
                }
                prefix |= digit << lo;
            }
            unsigned long long S = 0;
            sor_scan(j.g, cx, cy, cz, r, group, sub, tile, seg_pre, seg_off, [&](const CellPt &p) {
                const float d2 = sor_d2(q.x, q.y, q.z, p.x, p.y, p.z);
                if (fin && p.i != q.i && __float_as_uint(d2) < prefix) S += sor_u(d2);
            });
            S = sor_group_sum(S, group);
            if (fin) {
                S += (unsigned long long)(k - below) * sor_u(__uint_as_float(prefix));
                v = sor_v(S);
                active = false;
            }
        }
        if (mine && sub == 0) {
            j.v[q.i] = v;
            if (v == kSorNoScore) sIso++;
            else {
                uint64_t a, bhi, blo;
                sor_terms(v, a, bhi, blo);
                sM++; sA += a; sBhi += bhi; sBlo += blo;
            }
        }
    }
    sM = sor_wave_sum(sM); sA = sor_wave_sum(sA); sBhi = sor_wave_sum(sBhi); sBlo = sor_wave_sum(sBlo); sIso = sor_wave_sum(sIso); sRing = sor_wave_sum(sRing);
    if (lane == 0) {
        if (sM) { atomicAdd(&j.st[kSorM], sM); atomicAdd(&j.st[kSorA], sA); atomicAdd(&j.st[kSorBhi], sBhi); atomicAdd(&j.st[kSorBlo], sBlo); atomicAdd(&j.st[kSorSelected], sM); }
        if (sIso) atomicAdd(&j.st[kSorIsolated], sIso);
        if (sRing) atomicAdd(&j.st[kSorRingSum], sRing);
    }
}

__global__ __launch_bounds__(kSorT) void k_sor_flag(const SorJob *jobs)
{
    const SorJob &j = jobs[blockIdx.y];
    const long long base = (long long)blockIdx.x * kSorKeepTile;
    if (base >= j.g.n) return;
    __shared__ unsigned l_n;
    if (threadIdx.x == 0) l_n = 0;
    __syncthreads();
    double mean, sd;
    const double thr = sor_threshold(j.st[kSorM], j.st[kSorA], j.st[kSorBhi], j.st[kSorBlo], j.mul, mean, sd);
    unsigned mine = 0;
    for (int r = 0; r < kSorKeepTile / kSorT; r++) {
        const long long i = base + r * kSorT + threadIdx.x;
        if (i >= j.g.n) break;
        const bool rejected = j.g.slot[i] == kCellNoSlot;     // no query wrote its score
        const unsigned v = rejected ? kSorNoScore : j.v[i];
        if (rejected) j.v[i] = v;
        const bool kp = sor_keep(v, thr);
        j.keep[i] = kp ? 1 : 0;
        mine += kp ? 1u : 0u;
    }
    if (mine) atomicAdd(&l_n, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        j.tile_n[blockIdx.x] = l_n;
        if (l_n) atomicAdd(&j.st[kSorKept], (unsigned long long)l_n);
    }
}

__global__ __launch_bounds__(kSorT) void k_sor_compact(const SorJob *jobs)
{
    const SorJob &j = jobs[blockIdx.y];
    const long long base = (long long)blockIdx.x * kSorKeepTile;
    if (base >= j.g.n) return;
    __shared__ unsigned long long wsum[kSorT / 64];
    unsigned long long before = 0, total;
    for (unsigned b = threadIdx.x; b < blockIdx.x; b += kSorT) before += j.tile_n[b];
    (void)cellgrid_block_scan<kSorT>(before, wsum, total);
    unsigned long long at = total;                        // kept points of the tiles in front: <= base, so every write below stays inside out[n]
    for (int r = 0; r < kSorKeepTile / kSorT; r++) {
        const long long i = base + r * kSorT + threadIdx.x;
        const bool kp = i < j.g.n && j.keep[i] != 0;
        const unsigned long long pos = cellgrid_block_scan<kSorT>(kp ? 1ull : 0ull, wsum, total);
        if (kp) j.out[at + pos] = j.g.pts[i];
        at += total;
    }
}

} // namespace lmono
