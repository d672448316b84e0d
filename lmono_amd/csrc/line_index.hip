// lmono_amd/csrc/line_index.hip -- the (scan line, azimuth bin) index of the two "last" feature clouds that the odometry's searches sweep.
//
//   lb_key / az_bin / line_of / elev_of   what a point's bucket and elevation are: shared by the builders here and the searches (odometry.hip, corr_flat.hip)
//   li_reset / li_count / li_tables / li_scatter   the counting sort's steps over LDS counters, 16-bit (kHalf) or 32-bit wide
//   k_line_index<false>   the full-width launch: clouds of more than 65535 points, from the work list `li_todo` (normally empty)
// Every other cloud is indexed by k_compact_index (frontend.hip) with the 16-bit steps, while it writes the cloud.
#include "batch.hpp"

namespace lmono {

// Every candidate the searches ever accept lies closer than 5 m to the (transformed) feature point, i.e. within +-asin(r / rho_xy)
// of its azimuth and within a few scan lines of its elevation.  The index is a copy of every "last" cloud sorted by (scan line,
// azimuth bin), made once per scan (counting sort in LDS), and the start of every (line, bin) bucket: the candidates of a ball are ONE
// contiguous run per scan line -- a handful of short coalesced sweeps instead of a pass over whole scan lines.  A point of the copy carries
// (cloud index << 7 | line) in .w, the low word of the searches' u64 keys.
// Round 4 measured the (bin, line)-major order beside this one (commit 9c24d9d holds both behind LMONO_LB_ORDER; profiles/r4/NOTES.md section 1):
// equal for the chunked search (0.250 against 0.236 ms per launch), 3.0 instead of 2.2 ms per pass to build (a ring's consecutive points land 66
// buckets apart: scattered 16-B writes).  Removed again.
constexpr int kAzBins = 384;           // 0.9375 deg: about one point of a 0.2 m-voxelised cloud per bin and line at 12 m
constexpr int kLineKeys = 66 * kAzBins;
__device__ __forceinline__ int lb_key(int bin, int line) { return line * kAzBins + bin; }
constexpr int kLbPad = 4;              // entries behind the index copies: k_corr_flat's 64-B chunks may read up to three points past a run
// the runs of the copy that hold the lines va .. vb of the bins [b_lo, b_lo + nbins) (wrapping past the last bin): f(first point, count).
// Fall-back kernels only: simple beats fast.
template <class F>
__device__ __forceinline__ void lb_for_runs(const int *table, int b_lo, int nbins, int va, int vb, F f)
{
    const int b_end = b_lo + nbins;
    for (int part = 0; part < 2; part++) {
        if (part == 1 && b_end <= kAzBins) break;
        const int p0 = part ? 0 : b_lo, p1 = part ? b_end - kAzBins : min(b_end, kAzBins);
        for (int v = va; v <= vb; v++) { const int s0 = table[v * kAzBins + p0]; f(s0, table[v * kAzBins + p1] - s0); }
    }
}

__device__ __forceinline__ int az_bin(float x, float y)
{
    const float t = (atan2f(y, x) + 3.14159265f) * (kAzBins / 6.28318531f);
    const int bi = (int)t;
    return bi < 0 ? 0 : (bi >= kAzBins ? kAzBins - 1 : bi);
}
__device__ __forceinline__ int line_of(float w)
{
    const int v = (int)w;
    return v < 0 ? 0 : (v > 65 ? 65 : v);
}
// elevation angle of a point as the index sees it (only ever compared with margins: no exactness requirement on atan2f)
__device__ __forceinline__ float elev_of(float x, float y, float z) { return atan2f(z, sqrtf(x * x + y * y)); }
// order-preserving float <-> int map for LDS atomicMin / atomicMax
__device__ __forceinline__ int f2ord(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ float ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

constexpr int kLiT = 1024;     // threads of k_line_index and k_compact_index
constexpr int kLiLdsHalf = kLineKeys * 2, kLiLdsFull = kLineKeys * 4;   // dynamic LDS: one 16-bit / 32-bit counter per (line, bin)
constexpr int kLiBigGrid = 64;

// One (scan, cloud): copy of the cloud counting-sorted by (line, azimuth bin), the (line, bin) start table, per-line elevation bounds.
// kHalf: the counters are 16-bit halves of 32-bit LDS words (50 KB instead of 101 KB: more workgroups per CU -- the kernel is bound
// by its own dependent rounds, not by bytes); a cloud of more than 65535 points cannot be counted in 16 bits and goes through the
// work list `li_todo` to the full-width launch (small fixed grid, normally empty).
// The steps, each by every thread of the workgroup: li_reset | barrier | li_count for every point | barrier | li_tables | barrier |
// li_scatter.  k_line_index reads the cloud for the count; k_compact_index counts while compact_scan writes the cloud.
struct LiLds { int *cnt, *wsum, *emin, *emax; };      // counters (dynamic LDS), the waves' sums, the lines' elevation bounds (66 each)

// counter `key`: add one, return the old value
template <bool kHalf>
__device__ __forceinline__ int li_bump(const LiLds &L, int key)
{
    if (kHalf) { const int sh = (key & 1) * 16; return (int)((atomicAdd((unsigned int *)L.cnt + (key >> 1), 1u << sh) >> sh) & 0xffffu); }
    return atomicAdd(&L.cnt[key], 1);
}

template <bool kHalf>
__device__ __forceinline__ void li_reset(const LiLds &L)
{
    const int tid = threadIdx.x;
    constexpr int kWords = kHalf ? kLineKeys / 2 : kLineKeys;
    static_assert(kLineKeys % 2 == 0, "two 16-bit counters per LDS word");
    for (int i = tid; i < kWords; i += kLiT) L.cnt[i] = 0;
    if (tid < 66) { L.emin[tid] = INT_MAX; L.emax[tid] = INT_MIN; }
}

// one point per lane of a WHOLE wave (ok = false: a lane without one).  A wave holds 64 consecutive points, which nearly always
// share one scan line: their elevation bounds are reduced in the wave (DPP) and leave as ONE pair of LDS atomics
template <bool kHalf>
__device__ __forceinline__ void li_count(const LiLds &L, bool ok, float x, float y, float z, float w)
{
    const int ln = line_of(w);
    if (ok) (void)li_bump<kHalf>(L, lb_key(az_bin(x, y), ln));
    const unsigned long long act = __ballot(ok);
    if (act == 0ull) return;
    const int eo = f2ord(elev_of(x, y, z));
    const int ln0 = __shfl(ln, __ffsll((long long)act) - 1);
    if (__ballot(ok && ln != ln0) == 0ull) {
        const unsigned int lo = wave_min_u32_uniform(ok ? (unsigned int)eo ^ 0x80000000u : ~0u);
        const unsigned int hi = wave_max_u32_uniform(ok ? (unsigned int)eo ^ 0x80000000u : 0u);
        if ((threadIdx.x & 63) == 0) { atomicMin(&L.emin[ln0], (int)(lo ^ 0x80000000u)); atomicMax(&L.emax[ln0], (int)(hi ^ 0x80000000u)); }
    } else if (ok) {
        atomicMin(&L.emin[ln], eo);
        atomicMax(&L.emax[ln], eo);
    }
}

// the elevation rows and the start table of the counted cloud; the counters become the buckets' write cursors.  Holds barriers.
template <bool kHalf>
__device__ __forceinline__ void li_tables(const BatchView &b, const LiLds &L, int s, bool surf, int n)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int *table = b.lb_start + (size_t)(s * 2 + (surf ? 1 : 0)) * (kLineKeys + 1);
    unsigned int *s_c32 = (unsigned int *)L.cnt;
    // per-line elevation bounds of the cloud (empty line: lo > hi), used by the searches to bound the lines a ball can meet:
    // (lo, hi, A = min of lo over lines <= v, B = max of hi over lines >= v).  A and B are monotone (non-increasing in v) whatever
    // the sensor, so the lines that can meet an elevation window [a, b] lie between the first v with A_v <= b and the last with B_v >= a
    if (tid < 66) {
        float4 *el = b.lb_elev + (size_t)(s * 2 + (surf ? 1 : 0)) * 66;
        float A = 1e30f, B = -1e30f;
        for (int v = 0; v <= tid; v++) if (L.emin[v] != INT_MAX) A = fminf(A, ord2f(L.emin[v]));
        for (int v = tid; v < 66; v++) if (L.emin[v] != INT_MAX) B = fmaxf(B, ord2f(L.emax[v]));
        el[tid] = L.emin[tid] == INT_MAX ? make_float4(1e30f, -1e30f, A, B) : make_float4(ord2f(L.emin[tid]), ord2f(L.emax[tid]), A, B);
    }
    // exclusive prefix over the kLineKeys counters: kPer consecutive counters per thread (kPer even: whole LDS words; last threads padded)
    constexpr int kPer = (((kLineKeys + kLiT - 1) / kLiT) + 1) & ~1;
    auto get = [&](int idx) -> int { return kHalf ? (int)((s_c32[idx >> 1] >> ((idx & 1) * 16)) & 0xffffu) : L.cnt[idx]; };
    int local = 0;
    for (int i = 0; i < kPer; i++) { const int idx = tid * kPer + i; if (idx < kLineKeys) local += get(idx); }
    const int incl = wave_scan_incl(local);
    if (lane == 63) L.wsum[wave] = incl;
    __syncthreads();
    int run = incl - local;
    for (int w = 0; w < wave; w++) run += L.wsum[w];
    if (kHalf) {
        // a thread owns whole words (kPer is even): no other thread touches them here.  Cursors are < n <= 65535.
        for (int i = 0; i < kPer; i += 2) {
            const int idx = tid * kPer + i;
            if (idx < kLineKeys) {
                const unsigned int wv = s_c32[idx >> 1];
                const int c0 = (int)(wv & 0xffffu), c1 = (int)(wv >> 16);
                s_c32[idx >> 1] = (unsigned int)run | ((unsigned int)(run + c0) << 16);
                run += c0 + c1;
            }
        }
        // the table leaves LDS in rows (a wave writes 512 consecutive bytes; a thread's own counters lie 104 B apart): the cursors are the
        // buckets' starts until the scatter moves them
        __syncthreads();
        for (int w = tid; w < kLineKeys / 2; w += kLiT) { const unsigned int wv = s_c32[w]; table[2 * w] = (int)(wv & 0xffffu); table[2 * w + 1] = (int)(wv >> 16); }
    } else {
        for (int i = 0; i < kPer; i++) {
            const int idx = tid * kPer + i;
            if (idx < kLineKeys) { const int cnt = L.cnt[idx]; L.cnt[idx] = run; table[idx] = run; run += cnt; }
        }
    }
    if (tid == kLiT - 1) table[kLineKeys] = n;
}

// every point of the cloud to the next free place of its bucket
template <bool kHalf>
__device__ __forceinline__ void li_scatter(const BatchView &b, const LiLds &L, int s, bool surf, int n)
{
    const int tid = threadIdx.x;
    const float4 *src = surf ? b.less_flat + b.off[s] : b.less_sharp + (size_t)s * kMaxLessSharp;
    float4 *dst = surf ? b.lbs_pts + b.off[s] : b.lbc_pts + (size_t)s * kMaxLessSharp;
    for (int i0 = tid; i0 < n; i0 += 4 * kLiT) {
        float4 p[4];
#pragma unroll
        for (int q = 0; q < 4; q++) { const int i = i0 + kLiT * q; p[q] = src[i < n ? i : 0]; }      // unconditional (clamped): really four in flight
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = i0 + kLiT * q;
            if (i < n) {
                const int ln = line_of(p[q].w);
                const int d = li_bump<kHalf>(L, lb_key(az_bin(p[q].x, p[q].y), ln));
                dst[d] = make_float4(p[q].x, p[q].y, p[q].z, __int_as_float((i << 7) | ln));
            }
        }
    }
}

// the whole of it, full width, for a cloud that lies in memory
__device__ __forceinline__ void line_index_cloud(const BatchView &b, int s, bool surf, int n, const LiLds &L)
{
    const int tid = threadIdx.x;
    const float4 *src = surf ? b.less_flat + b.off[s] : b.less_sharp + (size_t)s * kMaxLessSharp;
    li_reset<false>(L);
    __syncthreads();
    // four points per thread and round, their loads in flight together
    for (int base = 0; base < n; base += 4 * kLiT) {      // uniform trip count: the wave reductions need every lane
        float4 p[4];
#pragma unroll
        for (int q = 0; q < 4; q++) { const int i = base + tid + kLiT * q; p[q] = src[i < n ? i : 0]; }      // unconditional (clamped): really four in flight
#pragma unroll
        for (int q = 0; q < 4; q++) li_count<false>(L, base + tid + kLiT * q < n, p[q].x, p[q].y, p[q].z, p[q].w);
    }
    __syncthreads();
    li_tables<false>(b, L, s, surf, n);
    __syncthreads();
    li_scatter<false>(b, L, s, surf, n);
}

// kLiBigGrid workgroups over the list of the clouds that 16-bit counters cannot count.  (A template for its one instantiation: the kernel's name says which width it is.)
template <bool kHalf>
__global__ __launch_bounds__(kLiT) void k_line_index(BatchView b)
{
    static_assert(!kHalf, "the 16-bit index is built by k_compact_index");
    extern __shared__ __align__(16) int s_cnt[];      // points per (line, bin); after the prefix: write cursor of the bucket
    __shared__ int s_wsum[kLiT / 64], s_emin[66], s_emax[66];
    const LiLds L = { s_cnt, s_wsum, s_emin, s_emax };
    const int n_todo = b.li_todo[0];
    for (int k = blockIdx.x; k < n_todo; k += gridDim.x) {
        const int e = b.li_todo[1 + k];
        __syncthreads();                            // the previous cloud's scatter is done with the counters
        line_index_cloud(b, e >> 1, (e & 1) != 0, b.feat_n[(e >> 1) * 4 + ((e & 1) ? 3 : 1)], L);
    }
}

} // namespace lmono
