// lmono_amd/csrc/corr_flat.hip -- laserOdometry correspondence search as FLATTENED candidate sweeps.
//
// Same results as k_correspond (odometry.hip): the exact nearest point (float distance, lowest index on ties) of every de-skewed
// feature point in the previous scan's less-sharp / less-flat cloud, then the reference's scan-line walk.
//
// Measured (profiles/r2/NOTES.md): giving a feature point 32 lanes (k_correspond), 16 lanes over an LDS tile or 4 lanes all cost ~440
// vector instructions per feature -- the lanes idle while a few dozen candidates are visited in short, ragged runs -- and one lane per
// feature with its own loops is bound by chains of dependent loads and by the slowest lane.  Here the ragged work of a workgroup's
// feature points is flattened through LDS, so that every lane always has a candidate:
//
//   round   1a  each feature's lane (the "owner") turns its search ball into run REQUESTS, one packed 32-bit word each: (line, first bin,
//               bins) of the (scan line, azimuth bin)-sorted copy of the cloud (k_line_index).  The ball's window of lines v1 .. v2 is
//               CARRIED in registers from round to round and only ever extended (below); ONE pass reserves a slot (two when the arc
//               wraps) for every line of the window with one LDS atomic add and posts: the line's run where the ball can meet the
//               line's own elevation range, an empty request (word 0) where it cannot
//           1b  the workgroup resolves all requests together (every lane kCfPer consecutive request words read as 8-byte pairs, 2 kCfPer
//               independent table loads in flight from ONE wave-uniform table base with 32-bit offsets: the less-flat cloud's table
//               lies kLineKeys + 1 entries behind the less-sharp one's) into runs (start, length), cuts every run into CHUNKS of
//               kCfC = 4 consecutive points and takes the exclusive prefix of the chunk counts WITHIN ITS WAVE; the waves' totals go
//               to LDS beside the descriptors
//           2   the chunks of ALL runs are one index space [0, C): every lane takes a contiguous range of chunks (the wave whose
//               runs hold its first chunk follows from the waves' totals, the run from a binary search over that wave's prefixes).
//               A chunk is 64 contiguous bytes: ONE address and four 16-B loads at immediate offsets, one owner, four distance
//               tests -- the run walk, the owner test and the address arithmetic are paid per chunk, not per candidate (round 3 dealt
//               single CANDIDATES to lanes: ~65 vector instructions per candidate, and the kernel is bound by instruction issue --
//               53 M VALU + 26 M SALU wave instructions per 256-chain launch, profiles/r4/NOTES.md).  The next chunk's descriptor
//               walk (LDS) runs while the current chunk's loads are in flight.  Every lane keeps the running minimum of the feature
//               its chunks belong to and posts it with one LDS atomic min per feature it touches
//           3   the owners read their minimum: settled (d <= r), or the radius grows and the feature joins the next round
//   then the same machinery runs the scan-line walk (lines ra-2 .. ra+2, growing arcs, two minima per feature).
//
// FOUR barriers per round (profiles/r7/NOTES.md; six before): behind 1a (requests and their count complete), behind 1b (descriptors
// and wave totals complete), behind 2 (minima complete), and the vote, which is also the barrier in front of the next round's 1a.
//   - no barrier for resetting the request counter: two counters alternate by the round's parity.  Round k posts to n_pool[k & 1]
//     and reads it in 1b; its thread 0 zeroes the OTHER counter in 1b, i.e. behind the barrier that follows 1a of round k (all uses of
//     that counter belong to round k - 1 and lie before it) and before the vote of round k (its next use is 1a of round k + 1)
//   - no barrier between the wave totals and the descriptors: the prefixes in the descriptors are per wave, so a lane writes its
//     descriptors without reading another wave's total; both are read only behind the one barrier after 1b
//   - the requests are written behind the vote of the previous round and were last read before that round's 1b barrier; the minima
//     are read by their owners behind the barrier after 2 and reset (walk) by the same owners in 1a
//
// Exactness: a point p with |p - q| <= r lies within asin(r / rho_xy(q)) of q's azimuth and within asin(r / |q|) of q's elevation
// angle; lb_elev holds every line's elevation range (lo, hi) and the envelopes A_v = min of lo over lines <= v, B_v = max of hi over
// lines >= v, both non-increasing in v.  A line that can meet the elevation window [elo, ehi] has lo <= ehi and hi >= elo, hence
// A_v <= ehi and B_v >= elo: it lies in v1 .. v2 with v1 = min{v : A_v <= ehi}, v2 = max{v : B_v >= elo}, and each line of the
// window is tested against its own range.  A feature's radius never shrinks over its rounds (r becomes 1.0005 x the distance just
// found, which was > 0.9999 r, or 2.5 r; a round in which it could not post keeps r), so ehi only rises and elo only falls, and because A and B are
// monotone v1 can only fall and v2 only rise: stepping the carried v1 down while A_(v1 - 1) <= ehi and v2 up while B_(v2 + 1) >= elo
// ends at exactly the two extrema above (the first window is reached the same way from the feature's own scan line).  Had a window
// ever been wider than that, only empty requests would be added: the per-line test decides what is searched.  A search of radius r
// is exact when its minimum is <= r.  Features whose reservation does not fit the round's pool post in the next round (the largest
// reservation, 66 lines x 2 pieces, fits an empty pool: no ball is too large for the flat search).
#include "batch.hpp"

namespace lmono {

#ifndef LMONO_CF_T
#define LMONO_CF_T 128
#endif
constexpr int kCfT = LMONO_CF_T;               // threads per workgroup = feature points per workgroup
constexpr int kCfBlocks = kMaxQueries / kCfT; // workgroups per chain
static_assert(kMaxQueries % kCfT == 0, "feature capacity must be a multiple of the workgroup size");
static_assert(kCfBlocks == kThinBlocks, "k_lm_solve skips the records of the workgroups a thinned lead-in pair does not run");
#ifndef LMONO_CF_PER
#define LMONO_CF_PER 6          // runs per lane and round (round 3, one run per LINE: 10)
#endif
#ifndef LMONO_CF_WAVES
#define LMONO_CF_WAVES 1
#endif
constexpr int kCfPer = LMONO_CF_PER;           // runs per lane and round
constexpr int kCfPool = kCfT * kCfPer;        // run descriptors per round
// first search radius of an unseeded feature (m): the less-sharp cloud is sparse (<= 20 points per ring and sector), the 0.2 m-voxelised
// less-flat cloud dense.  Any value is exact; measured per bench step: (0.3, 0.3) 49.0 ms, (0.5, 0.3) 48.8, (0.5, 0.2) 48.1, (0.5, 0.15) 47.8,
// (0.5, 0.1) 48.4, (0.8, 0.3) 49.0; a term proportional to the range did not help.
#ifndef LMONO_R0_PLANE
#define LMONO_R0_PLANE 0.25f
#define LMONO_R0_EDGE 0.7f
#endif
constexpr float kCfR0Edge = LMONO_R0_EDGE, kCfR0Plane = LMONO_R0_PLANE;
constexpr int kCfC = 4;                        // points per chunk (64 contiguous bytes)
#ifndef LMONO_CF_B
#define LMONO_CF_B 2
#endif
constexpr int kCfB = LMONO_CF_B;               // chunks per lane in flight (kCfB x kCfC 16-B loads)
static_assert(kCfC - 1 <= kLbPad, "a chunk's loads may run kCfC - 1 points past its run: the index copies are padded");
// Round budgets of the two phases: a workgroup runs as many rounds as its SLOWEST feature needs, and a launch lasts as long as its slowest
// workgroup; a feature that has not settled within the budget goes to the device work list of k_correspond_list (exact as well).
#ifndef LMONO_CF_NN_ROUNDS
#define LMONO_CF_NN_ROUNDS 64
#define LMONO_CF_WALK_ROUNDS 64
#endif
constexpr int kCfNnRounds = LMONO_CF_NN_ROUNDS, kCfWalkRounds = LMONO_CF_WALK_ROUNDS;

// run request, one word: line (7 bits) | first bin (9) << 7 | bins (9) << 16 | owner (7) << 25.  The cloud follows from the owner.
__device__ __forceinline__ unsigned int cf_request_line(int line, int b0, int nb, int owner) { return (unsigned int)line | ((unsigned int)b0 << 7) | ((unsigned int)nb << 16) | ((unsigned int)owner << 25); }
static_assert(kCfT <= 128 && kAzBins <= 511, "request packing");       // (owner 7 bits, bins 9 bits)
static_assert(66 * 2 <= kCfPool, "a nearest-point reservation (every line of the window, two pieces when the arc wraps) fits the pool");

struct CfRun {                                // resolved run
    unsigned int start;                       // first point of the run in its index copy
    unsigned int pre;                         // chunks before this run among the runs its wave resolved (CfLds::wsum holds the waves' totals)
    unsigned short len;                       // points
    unsigned char owner;                      // feature (lane) the run belongs to
    unsigned char tag;                        // bit 7: surf cloud
};
static_assert(sizeof(CfRun) == 12, "run descriptor layout");

struct CfLds {
    float4 elev[2][66];                       // lb_elev of the two "last" clouds
    int fge[2][66], lle[2][66];
    float4 q[kCfT];                           // de-skewed feature points
    unsigned long long best[kCfT];            // nearest point: (d2 bits) << 32 | index << 7 | line (the low word is the index copy's .w)
    unsigned long long same[kCfT], other[kCfT];
    int closest[kCfT], wlo[kCfT], whi[kCfT];  // closest: index << 7 | line of the nearest point (the walk's centre line rides in the low bits)
    alignas(8) unsigned int req[kCfPool];
    CfRun pool[kCfPool];
    int n_pool[2];                            // requests posted in this round / the next one (by the round's parity)
    int wsum[kCfT / 64];                      // chunks of the runs each wave resolved
};

__device__ __forceinline__ void cf_defer(unsigned int *wl, int c, int qi)
{
    const unsigned int slot = atomicAdd(wl, 1u);
    wl[1 + slot] = ((unsigned int)c << 12) | (unsigned int)qi;
}

// azimuth arc of radius r around the feature: nb bins from bin a0 on, wrapping past the last bin
struct CfArc { int a0, nb; };
__device__ __forceinline__ void cf_arc(float r, float rho, float th, CfArc &a)
{
    constexpr float kb = kAzBins / 6.28318531f;
    a.a0 = 0; a.nb = kAzBins;
    if (!(rho > r * 1.002f)) return;                      // the ball reaches the sensor axis: every azimuth
    const float alpha = asin_upper(r / rho) + kArcSlackBins / kb;
    const int lo = (int)floorf((th - alpha) * kb), hi = (int)floorf((th + alpha) * kb);
    const int n = hi - lo + 1;
    if (n >= kAzBins) return;
    a.a0 = ((lo % kAzBins) + kAzBins) % kAzBins;
    a.nb = n;
}
// the arc on one line is one run, two when it wraps past the last bin
__device__ __forceinline__ int cf_arc_pieces(const CfArc &a) { return a.a0 + a.nb > kAzBins ? 2 : 1; }
__device__ __forceinline__ void cf_post_line(unsigned int *req, int &slot, const CfArc &a, int line, int owner)
{
    const int n0 = min(a.nb, kAzBins - a.a0);
    req[slot++] = cf_request_line(line, a.a0, n0, owner);
    if (n0 < a.nb) req[slot++] = cf_request_line(line, 0, a.nb - n0, owner);
}

// Line window of a ball: v1 = min{v : A_v <= ehi}, v2 = max{v : B_v >= elo} over the envelopes A (.z) and B (.w), both non-increasing in
// the line.  A feature's radius never shrinks over its rounds, so ehi only rises and elo only falls: v1 can only fall and v2 only rise.
// The window is CARRIED in registers and extended by stepping along the envelope, two independent LDS reads per step.
__device__ __forceinline__ void cf_window_start(const float4 *el, int s, float elo, float ehi, int &v1, int &v2)
{
    // from the feature's own scan line towards the window: afterwards A_v1 <= ehi or v1 == 66, B_v2 >= elo or v2 == -1
    v1 = s; v2 = s;
    while (v1 < 66 && el[v1].z > ehi) v1++;
    while (v2 >= 0 && el[v2].w < elo) v2--;
}
__device__ __forceinline__ void cf_window_extend(const float4 *el, float elo, float ehi, int &v1, int &v2)
{
    while (v1 > 0) {
        const float a1 = el[v1 - 1].z, a2 = el[max(v1 - 2, 0)].z;
        if (!(a1 <= ehi)) break;
        v1 -= (v1 >= 2 && a2 <= ehi) ? 2 : 1;
    }
    while (v2 < 65) {
        const float b1 = el[v2 + 1].w, b2 = el[min(v2 + 2, 65)].w;
        if (!(b1 >= elo)) break;
        v2 += (v2 <= 63 && b2 >= elo) ? 2 : 1;
    }
}

// stages 1b and 2 of a round, executed by the whole workgroup.  kWalk = false: nearest point (minimum into L.best);
// kWalk = true: scan-line walk (minima into L.same / L.other).
#ifdef LMONO_TILE_PROF
#define CF_STAMP(v) { if (threadIdx.x == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); (v) += t_ - cf_t; cf_t = t_; } }
#define CF_WAIT_VM() __builtin_amdgcn_s_waitcnt(0x0F70);     /* vmcnt(0): the stamp behind it sees the gathers arrive */
#define CF_COUNT(v) { if (threadIdx.x == 0) (v) += 1; }
#else
#define CF_STAMP(v)
#define CF_WAIT_VM()
#define CF_COUNT(v)
#endif

// `par` is the round's parity (the pool counter in use); `tg` is the cloud pair's bucket table (lb_start of the less-sharp cloud; the
// less-flat cloud's follows kLineKeys + 1 entries behind it).  Returns the round's number of chunks.
template <bool kWalk>
__device__ __forceinline__ int cf_sweep(CfLds &L, int par, int n_edge_owner, const int *tg, const float4 *pts_c, const float4 *pts_s, unsigned long long &cf_t, unsigned long long *cf_acc)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_pool = min(L.n_pool[par], kCfPool);
    if (tid == 0) L.n_pool[par ^ 1] = 0;            // the NEXT round's counter: last read before the previous round's prefix barrier, next used behind this round's vote
    // ---- 1b: resolve this lane's kCfPer consecutive requests (wide LDS reads; all table loads in flight together, ONE wave-uniform
    //          table base and a 32-bit byte offset per load), prefix of the chunk counts within the wave.  Words behind the round's
    //          requests resolve as empty requests (word 0: no bins), so nothing here is behind a branch.
    unsigned int rq[kCfPer], st[kCfPer], en[kCfPer];
    if constexpr (kCfPer % 2 == 0) {
        const uint2 *rp = (const uint2 *)&L.req[tid * kCfPer];          // 8-byte aligned: kCfPer is even
#pragma unroll
        for (int j = 0; j < kCfPer / 2; j++) { const uint2 w2 = rp[j]; rq[2 * j] = w2.x; rq[2 * j + 1] = w2.y; }
    } else {
#pragma unroll
        for (int j = 0; j < kCfPer; j++) rq[j] = L.req[tid * kCfPer + j];
    }
    const char *tgb = (const char *)uni_ptr(tg);
#pragma unroll
    for (int j = 0; j < kCfPer; j++) {
        if (tid * kCfPer + j >= n_pool) rq[j] = 0u;
        const unsigned int own = rq[j] >> 25;
        const unsigned int e0 = (rq[j] & 127u) * (unsigned int)kAzBins + ((rq[j] >> 7) & 511u) + ((int)own >= n_edge_owner ? (unsigned int)(kLineKeys + 1) : 0u);
        unsigned int b0 = e0 * 4u, b1 = b0 + ((rq[j] >> 16) & 511u) * 4u;
        asm volatile("" : "+v"(b1));                // (keeps the second load on the scalar base + 32-bit offset form: otherwise the sum is re-split into 64-bit adds)
        st[j] = *(const unsigned int *)(tgb + b0); en[j] = *(const unsigned int *)(tgb + b1);
    }
    int sum = 0;
#pragma unroll
    for (int j = 0; j < kCfPer; j++) { en[j] = min(en[j] - st[j], 65535u); sum += (int)((en[j] + kCfC - 1) / kCfC); }      // en = length from here on
    const int incl = wave_scan_incl(sum);
    if (lane == 63) L.wsum[wave] = incl;
    int run = incl - sum;
#pragma unroll
    for (int j = 0; j < kCfPer; j++) {
        const unsigned int own = rq[j] >> 25;
        CfRun d;
        d.start = st[j]; d.pre = (unsigned int)run; d.len = (unsigned short)en[j];
        d.owner = (unsigned char)own; d.tag = (unsigned char)((int)own >= n_edge_owner ? 0x80 : 0);
        L.pool[tid * kCfPer + j] = d;               // every descriptor of the pool is valid: the ones behind the round's requests are empty runs
        run += (int)((en[j] + kCfC - 1) / kCfC);
    }
    __syncthreads();
    CF_STAMP(cf_acc[1])
    // ---- 2: this lane's contiguous range of chunks
    int C = 0;
#pragma unroll
    for (int w = 0; w < kCfT / 64; w++) C += L.wsum[w];
    if (C <= 0) return C;
    const int ch = (C + kCfT - 1) / kCfT;
    int j = tid * ch;
    const int j1 = min(j + ch, C);
    if (j >= j1) return C;
    // run that holds chunk j: the wave whose runs hold it (the prefixes are per wave), then the last of that wave's runs with
    // pre <= j - (chunks of the waves before it) (runs without chunks share their pre with the next run)
    int seg, jl = j;
    {
        int w = 0;
#pragma unroll
        for (int i = 0; i + 1 < kCfT / 64; i++) { const int sw = L.wsum[i]; if (w == i && jl >= sw) { jl -= sw; w = i + 1; } }
        int lo = w * 64 * kCfPer, hi = lo + 64 * kCfPer - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if ((int)L.pool[mid].pre <= jl) lo = mid; else hi = mid - 1; }
        seg = lo;
    }
    CfRun cur = L.pool[seg];
    int off = (jl - (int)cur.pre) * kCfC;          // first point of the chunk inside its run
    CF_STAMP(cf_acc[10])
    int owner = -1;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    unsigned long long m0 = ~0ull, m1 = ~0ull;      // running minima of the current owner (nearest / same, other)
    int closest = 0, w_lo = 0, ra = 0;
    unsigned int w_span = 0;
    constexpr bool wk = kWalk;
    auto flush = [&]() {
        if (owner < 0) return;
        if (!wk) { if (m0 != ~0ull) atomicMin(&L.best[owner], m0); }
        else { if (m0 != ~0ull) atomicMin(&L.same[owner], m0); if (m1 != ~0ull) atomicMin(&L.other[owner], m1); }
    };
    // the kCfB chunks (first point, live points, owner) the loop body works on; the NEXT ones are prepared while these loads are in flight
    const float4 *pp[kCfB]; int n[kCfB], ow[kCfB];
#pragma unroll
    for (int bb = 0; bb < kCfB; bb++) { pp[bb] = pts_c; n[bb] = 0; ow[bb] = -1; }
    auto next_chunks = [&]() {
#pragma unroll
        for (int bb = 0; bb < kCfB; bb++) {
            n[bb] = 0;                                    // no chunk left: the loads read a valid dummy, nothing is live
            if (j < j1) {
                while (off >= (int)cur.len) { seg++; cur = L.pool[seg]; off = 0; }
                pp[bb] = ((cur.tag & 0x80) ? pts_s : pts_c) + cur.start + off;
                n[bb] = (int)cur.len - off; ow[bb] = cur.owner;
                off += kCfC; j++;
            }
        }
    };
    next_chunks();
    for (;;) {
        // UNCONDITIONAL loads at immediate offsets (the copies are padded: a chunk may run up to three points past its run; the
        // points behind the run's end are masked below).  Behind a branch the compiler would wait for each load in turn (round 3).
        float4 p[kCfB][kCfC];
#pragma unroll
        for (int bb = 0; bb < kCfB; bb++)
#pragma unroll
            for (int u = 0; u < kCfC; u++) p[bb][u] = pp[bb][u];
        __builtin_amdgcn_sched_barrier(0);          // everything below stays below the loads
        CF_STAMP(cf_acc[11])
        int n_c[kCfB], ow_c[kCfB];
#pragma unroll
        for (int bb = 0; bb < kCfB; bb++) { n_c[bb] = n[bb]; ow_c[bb] = ow[bb]; }
        const bool more = j < j1;
        if (more) next_chunks();
        CF_WAIT_VM()
        CF_STAMP(cf_acc[12])
        CF_COUNT(cf_acc[15])
#pragma unroll
        for (int bb = 0; bb < kCfB; bb++) {
            if (n_c[bb] > 0 && ow_c[bb] != owner) {
                CF_COUNT(cf_acc[16])
                flush();
                owner = ow_c[bb]; m0 = ~0ull; m1 = ~0ull;
                const float4 qq = L.q[owner];
                qx = qq.x; qy = qq.y; qz = qq.z;
                if (wk) { const int cr = L.closest[owner]; closest = cr >> 7; ra = cr & 127; w_lo = L.wlo[owner]; w_span = (unsigned int)(L.whi[owner] - w_lo); }
            }
#pragma unroll
            for (int u = 0; u < kCfC; u++) {
                const float4 pt = p[bb][u];
                const float d = dist2f(pt.x, pt.y, pt.z, qx, qy, qz);
                const int pw = __float_as_int(pt.w);      // cloud index << 7 | line
                const bool live = u < n_c[bb];
                if (!wk) {
                    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned int)pw;
                    m0 = (live & (key < m0)) ? key : m0;
                } else {
                    const int jj = pw >> 7, dv = (pw & 127) - ra, sj = jj - closest;
                    const bool ok = live & (sj != 0) & ((unsigned int)(jj - w_lo) < w_span);          // inside the window the reference's loops can reach
                    const unsigned int seq = sj > 0 ? (unsigned int)(sj - 1) : kSeqBack + (unsigned int)(-1 - sj);
                    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | seq;
                    const bool is_other = sj > 0 ? (dv > 0) : (dv < 0);       // ra = the nearest point's own line (an edge feature's "same" minimum is never read)
                    m1 = (ok & is_other & (key < m1)) ? key : m1;
                    m0 = (ok & !is_other & (key < m0)) ? key : m0;
                }
            }
        }
        CF_STAMP(cf_acc[13])
        if (!more) break;
    }
    flush();
    CF_STAMP(cf_acc[14])
    return C;
}

// step `step`, outer iteration `outer` of every chain: kCfBlocks workgroups of kCfT feature points per chain (measured: 256 threads
// 30.0 ms of correspondence search per bench step, 128 threads 26.6, 64 threads 31.4; 4 or 8 gathers in flight make no difference), decoded onto ONE XCD
// per chain (blocks b and b + 8 share an XCD): the chain's index and tables are fetched into one L2 only.
__global__ __launch_bounds__(kCfT, LMONO_CF_WAVES) void k_corr_flat(BatchView b, OdomView o, int step, int outer, unsigned int *wl, int defer_every, unsigned long long *stats)
{
    __shared__ CfLds L;
    const int xcd = blockIdx.x & 7, u = blockIdx.x >> 3;
    const int ci = o.chain0 + (u / kCfBlocks) * 8 + xcd;
    const int qb = u % kCfBlocks;
    if (ci >= o.chain1) return;
    const int c = o.clist ? o.clist[ci] : ci;
    int own;
    const int k = chain_scan(o, c, step, own);
    if (k < 0) return;
    if (lead_in_thinned(o, k, own) && qb % kThinStride != 0) return;      // early lead-in pair: every kThinStride-th share of the features
    const int tid = threadIdx.x;
    const int l = k - 1;
    const int n_sharp = b.feat_n[k * 4 + 0];
    const int nq = n_sharp + b.feat_n[k * 4 + 2];
    if (qb >= nq) return;
    // the chain's features are dealt round-robin over its kCfBlocks workgroups: every workgroup gets the same share of edge and plane
    // features (blocks of consecutive features gave workgroups of very different weight, and an almost empty last one)
    const int qi = tid * kCfBlocks + qb;
    if (b.status[l] & (kStatusIrregularLines | kStatusDenseCell)) {
        if (qi < nq) cf_defer(wl, c, qi);       // rare: the whole scan pair goes to the generic search
        return;
    }
    // the feature point and its seed are requested before the small tables are staged
    const bool edge = qi < n_sharp;
    const int cl = edge ? 0 : 1;
    const int n_edge_owner = n_sharp > qb ? (n_sharp - qb + kCfBlocks - 1) / kCfBlocks : 0;      // owners (lanes) below it hold edge features
    float4 fp = make_float4(0.f, 0.f, 0.f, 0.f);
    int *seed_c = o.seed ? o.seed + (size_t)c * kMaxQueries : nullptr;
    int sidx = -1;
    if (qi < nq) {
        fp = edge ? b.sharp[(size_t)k * kMaxSharp + qi] : b.flat[(size_t)k * kMaxFlat + (qi - n_sharp)];
        if (outer == 1 && seed_c) sidx = seed_c[qi];
    }
    // second outer iteration: the partners the walk found in the first one bound its radius (below)
    int4 prev = make_int4(-1, -1, -1, 0);
    if (qi < nq && outer == 1 && seed_c && sidx >= 0) prev = ((const int4 *)o.corr + (size_t)c * kMaxQueries)[qi];
    // the two clouds' tables lie behind each other in HBM as in LDS: flat copies of 2 x 66 entries
    for (int xx = tid; xx < 2 * 66; xx += kCfT) {
        (&L.elev[0][0])[xx] = b.lb_elev[(size_t)l * (2 * 66) + xx];
        (&L.fge[0][0])[xx] = b.line_first_ge[(size_t)l * (2 * 66) + xx];
        (&L.lle[0][0])[xx] = b.line_last_le[(size_t)l * (2 * 66) + xx];
    }
    if (tid == 0) { L.n_pool[0] = 0; L.n_pool[1] = 0; }
    const int n_last = b.feat_n[l * 4 + (edge ? 1 : 3)];
    const float4 *cloud = edge ? b.less_sharp + (size_t)l * kMaxLessSharp : b.less_flat + b.off[l];
    float4 sp = make_float4(0.f, 0.f, 0.f, 0.f);
    if (sidx >= 0 && sidx < n_last) sp = cloud[sidx]; else sidx = -1;
    // de-skew transform in fp64 as the reference's TransformToStart
    const double *x = o.state + c * 8;
    double rx, ry, rz;
    quat_rotate(x, (double)fp.x, (double)fp.y, (double)fp.z, rx, ry, rz);
    const float qx = (float)(rx + x[4]), qy = (float)(ry + x[5]), qz = (float)(rz + x[6]);
    float sd = -1.0f;
    if (sidx >= 0) { const float d = dist2f(sp.x, sp.y, sp.z, qx, qy, qz); if (d < 24.0f) sd = d; }
    L.q[tid] = make_float4(qx, qy, qz, 0.f);
    L.best[tid] = ~0ull;
    const int *tg = b.lb_start + (size_t)(l * 2) * (kLineKeys + 1);      // less-sharp table; the less-flat one follows it
    const float4 *pts_c = b.lbc_pts + (size_t)l * kMaxLessSharp, *pts_s = b.lbs_pts + b.off[l];
    const float rho2 = qx * qx + qy * qy, rho = sqrtf(rho2), R = sqrtf(rho2 + qz * qz);
    const float th = atan2f(qy, qx) + 3.14159265f;
    const float eq = elev_of(qx, qy, qz);
    unsigned long long cf_t = 0, cf_acc[20] = { 0 };      // diagnostic build: cycles per stage (1a, 1b, 2, 3, setup, epilogue), rounds, candidates
#ifdef LMONO_TILE_PROF
    if (tid == 0) cf_t = __builtin_amdgcn_s_memtime();
#endif
    bool alive = qi < nq && n_last > 0;       // still looking for its nearest point
    bool deferred = false;
    if (defer_every > 0 && qi < nq && qi % defer_every == 0) { alive = false; deferred = true; }      // test hook: exercise the fall-back kernel
    float r = sd >= 0.f ? sqrtf(sd) * 1.0005f + 1e-3f : (edge ? kCfR0Edge : kCfR0Plane);
    __syncthreads();
    int par = 0;                              // parity of the round: which of the two pool counters it posts to
    // the line window of the first ball, approached from the feature's own scan line; the rounds only ever extend it
    int v1 = 66, v2 = -1;
    auto elev_window = [&](float rr, float &elo, float &ehi) {
        const float beta = R > rr ? asin_upper(rr / R) + 5e-4f : 4.0f;
        elo = eq - beta; ehi = eq + beta;
    };
    if (alive) {
        float elo, ehi;
        elev_window(fminf(r, 5.0f), elo, ehi);
        cf_window_start(L.elev[cl], line_of(fp.w), elo, ehi, v1, v2);
    }
    CF_STAMP(cf_acc[4])
    // ================= nearest point =================
#ifdef LMONO_TILE_PROF
    int my_rounds = 0;          // rounds THIS feature took part in (nearest point + walk): the workgroup runs max(nearest) + max(walk), a merged loop would run max of the sums
#endif
    for (int round = 0; round < kCfNnRounds; round++) {
#ifdef LMONO_TILE_PROF
        my_rounds += alive ? 1 : 0;
#endif
        // ---- 1a: run requests of the features still searching
        const float rr = fminf(r, 5.0f);                    // d2 < 25 means d < 5: a 5 m ball holds every admissible point
        bool posted = false;
        if (alive) {
            const float4 *el = L.elev[cl];
            CfArc a;
            cf_arc(rr, rho, th, a);
            float elo, ehi;
            elev_window(rr, elo, ehi);
            cf_window_extend(el, elo, ehi, v1, v2);
            // ONE pass: a slot (two when the arc wraps) is reserved for every line of the window v1 .. v2; the lines the ball can meet
            // post their run there, a line whose own range misses the ball an empty request (word 0: no bins, no chunks)
            const int pieces = cf_arc_pieces(a);
            const int nreq = max(v2 - v1 + 1, 0) * pieces;                 // <= 66 * 2 <= kCfPool
            int slot = nreq > 0 ? atomicAdd(&L.n_pool[par], nreq) : 0;
            if (slot + nreq <= kCfPool) {
                posted = true;
                const int n0 = min(a.nb, kAzBins - a.a0);
                const unsigned int w0 = cf_request_line(0, a.a0, n0, tid), w1 = cf_request_line(0, 0, a.nb - n0, tid);
                for (int v = v1; v <= v2; v++) {
                    const float4 ev = el[v];
                    const bool meet = !(ev.y < elo || ev.x > ehi);
                    L.req[slot++] = meet ? (w0 | (unsigned int)v) : 0u;
                    if (pieces == 2) L.req[slot++] = meet ? (w1 | (unsigned int)v) : 0u;
                }
            } else {
                // the pool of this round is full: the feature posts again in the next round; the part of its reservation that
                // lies inside the pool becomes empty runs
                for (int t = slot; t < kCfPool; t++) L.req[t] = 0u;
            }
        }
        __syncthreads();
        CF_STAMP(cf_acc[0])
        const int n_chunks = cf_sweep<false>(L, par, n_edge_owner, tg, pts_c, pts_s, cf_t, cf_acc);
        par ^= 1;                             // (also behind the last round: the walk's first round finds the counter this round zeroed)
        __syncthreads();
        CF_STAMP(cf_acc[2])
#ifdef LMONO_TILE_PROF
        if (tid == 0) { cf_acc[6] += 1; cf_acc[8] += (unsigned long long)n_chunks; }
#else
        (void)n_chunks;
#endif
        // ---- 3: owners decide
        if (alive && posted) {
            const unsigned long long best = L.best[tid];
            if (best != ~0ull) {
                const float bd = __uint_as_float((unsigned int)(best >> 32));
                if (bd <= (rr * 0.9999f) * (rr * 0.9999f) || rr >= 5.0f) alive = false;
                else r = sqrtf(bd) * 1.0005f + 1e-3f;
            } else {
                if (rr >= 5.0f) alive = false;
                else r = rr * 2.5f;
            }
        }
        CF_STAMP(cf_acc[3])
        if (!__syncthreads_or(alive ? 1 : 0)) break;
    }
    if (alive) { alive = false; deferred = true; }            // round budget exhausted (never observed): list kernel

    // ================= scan-line walk =================
    const unsigned long long nn = L.best[tid];
    const unsigned long long thr = pack_fu(25.0f, 0u);
    bool walking = qi < nq && n_last > 0 && !deferred && nn != ~0ull && (double)__uint_as_float((unsigned int)(nn >> 32)) < 25.0;
    const int closest = (int)((unsigned int)(nn & 0xffffffffull) >> 7);
    const int ra = (int)(nn & 127ull);
    if (walking) {
        L.closest[tid] = (closest << 7) | ra;
        L.wlo[tid] = ra - 3 >= 0 ? L.lle[cl][ra - 3] + 1 : 0;
        L.whi[tid] = ra + 3 <= 65 ? L.fge[cl][ra + 3] : n_last;
    }
    // radii: the neighbouring lines right next to the nearest point; the ring gap of far ground points (rho^2 dtheta / h); 5 m
    const float rad[4] = { walk_radius(0, rho), walk_radius(1, rho), walk_radius(2, rho), walk_radius(3, rho) };
    int wpass = 0;
    unsigned long long same = thr, other = thr;
    // Seeded walk: when the nearest point is the one of the first outer iteration, the partners found then are still admissible
    // candidates, so the new minima are no farther than they are: ONE pass with the ball that just holds them is exact (their own
    // keys are strictly inside it).  Otherwise, and if that pass does not settle, the radius ladder below runs as usual.
    float r_seed = -1.0f;
    if (walking && prev.w != 0 && prev.x == closest) {
        const int i_o = edge ? prev.y : prev.z;
        const float4 po = cloud[i_o];
        float d = dist2f(po.x, po.y, po.z, qx, qy, qz);
        if (!edge) { const float4 ps = cloud[prev.y]; d = fmaxf(d, dist2f(ps.x, ps.y, ps.z, qx, qy, qz)); }
        if (d < 24.0f) r_seed = sqrtf(d) * 1.002f + 1e-3f;
    }
    for (int round = 0; round < kCfWalkRounds; round++) {
#ifdef LMONO_TILE_PROF
        my_rounds += walking ? 1 : 0;
#endif
        bool posted = false;
        if (walking) {
            while (wpass > 0 && wpass < 4 && rad[wpass] <= rad[wpass - 1]) wpass++;
            if (wpass >= 4) walking = false;
        }
        const bool seeded = r_seed > 0.0f;
        const float r_now = seeded ? r_seed : rad[wpass < 4 ? wpass : 3];
        if (walking) {
            CfArc a;
            cf_arc(r_now, rho, th, a);
            // one run (two when the arc wraps) per line of ra-2 .. ra+2, without an edge feature's own line
            const int wv1 = max(ra - 2, 0), wv2 = min(ra + 2, 65);
            const int nreq = (wv2 - wv1 + 1 - (edge ? 1 : 0)) * cf_arc_pieces(a);
            int slot = atomicAdd(&L.n_pool[par], nreq);
            if (slot + nreq <= kCfPool) {
                posted = true;
                L.same[tid] = thr; L.other[tid] = thr;
                for (int v = wv1; v <= wv2; v++) if (!(edge && v == ra)) cf_post_line(L.req, slot, a, v, tid);
            } else
                for (int t = slot; t < kCfPool; t++) L.req[t] = 0u;
        }
        __syncthreads();
        CF_STAMP(cf_acc[0])
        const int n_chunks = cf_sweep<true>(L, par, n_edge_owner, tg, pts_c, pts_s, cf_t, cf_acc);
        par ^= 1;
        __syncthreads();
        CF_STAMP(cf_acc[2])
#ifdef LMONO_TILE_PROF
        if (tid == 0) { cf_acc[7] += 1; cf_acc[9] += (unsigned long long)n_chunks; }
#else
        (void)n_chunks;
#endif
        if (walking && posted) {
            same = L.same[tid]; other = L.other[tid];
            if (!seeded && r_now >= 5.0f) walking = false;
            else {
                const unsigned long long lim = pack_fu(r_now * r_now * 0.998f, 0u);     // strictly inside the ball of this pass
                if (other < lim && (edge || same < lim)) walking = false;
                else if (seeded) r_seed = -1.0f;          // (not expected) back to the ladder
                else {
                    wpass++;
                    while (wpass < 4 && rad[wpass] <= rad[wpass - 1]) wpass++;
                    // the pass SAW the partners it needs, but outside its ball (its arc's bins hold more than the ball): the ball that just holds
                    // them settles the walk exactly -- every point outside it is farther -- and is usually much smaller than the next rung's
                    if (other < thr && (edge || same < thr)) {
                        const float d = edge ? __uint_as_float((unsigned int)(other >> 32)) : fmaxf(__uint_as_float((unsigned int)(other >> 32)), __uint_as_float((unsigned int)(same >> 32)));
                        const float rt = sqrtf(d) * 1.002f + 1e-3f;
                        if (wpass < 4 && rt < rad[wpass] && d < 24.0f) r_seed = rt;
                    }
                }
            }
        }
        CF_STAMP(cf_acc[3])
        if (!__syncthreads_or(walking ? 1 : 0)) break;
    }
#ifdef LMONO_TILE_PROF
    {
        const int mr = __syncthreads_or(0) * 0 + my_rounds;
        __shared__ int s_maxr, s_sumr;
        if (tid == 0) { s_maxr = 0; s_sumr = 0; }
        __syncthreads();
        atomicMax(&s_maxr, mr); atomicAdd(&s_sumr, mr);
        __syncthreads();
        if (tid == 0) { cf_acc[17] = (unsigned long long)s_maxr; cf_acc[18] = (unsigned long long)s_sumr; }
    }
    if (tid == 0 && stats) { atomicAdd(&stats[1], 1ull); for (int i = 0; i < 20; i++) atomicAdd(&stats[2 + i], cf_acc[i]); }
#endif
    if (qi >= nq) return;
    if (deferred || walking) { cf_defer(wl, c, qi); return; }
    int4 rres = make_int4(-1, -1, -1, 0);
    int closest_out = -1;
    if (n_last > 0 && nn != ~0ull && (double)__uint_as_float((unsigned int)(nn >> 32)) < 25.0) {
        closest_out = closest;
        const int i_other = other < thr ? seq_to_index((unsigned int)(other & 0xffffffffull), closest) : -1;
        if (edge) { if (i_other >= 0) rres = make_int4(closest, i_other, -1, 1); }
        else {
            const int i_same = same < thr ? seq_to_index((unsigned int)(same & 0xffffffffull), closest) : -1;
            if (i_same >= 0 && i_other >= 0) rres = make_int4(closest, i_same, i_other, 2);
        }
    }
    ((int4 *)o.corr + (size_t)c * kMaxQueries)[qi] = rres;
    if (outer == 0 && seed_c) seed_c[qi] = closest_out;
    // residual-block record for the solver: the feature point and its 2 (edge) or 3 (plane) partners, staged (64 B)
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A, C = A;
    if (rres.w != 0) { A = cloud[rres.x]; B = cloud[rres.y]; if (rres.z >= 0) C = cloud[rres.z]; }
    fp.w = __int_as_float(rres.w);
    store_staged_record(o.crec + ((size_t)c * kMaxQueries + qi) * 4, fp, A, B, C);
}

} // namespace lmono
