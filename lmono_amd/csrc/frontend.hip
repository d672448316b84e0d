// lmono_amd/csrc/frontend.hip -- gfx950 kernels of the LiDAR front end (A-LOAM scanRegistration;
// source absent from the reference tree, behavioural spec SURVEY.md Appendix A.1).
//
// Four kernel stages per batch of scans over HBM-resident SoA/float4 pools:
//   k_ring_*     filter, ring id, azimuth, stable counting sort into ring-major order: four tile-parallel launches (ends, tag,
//                offsets, scatter); every wave owns a 1024-point segment in both passes, no barriers inside the passes; the tag
//                pass decides ring and half sweep without an arctangent (ring_decide.hpp), fp64 forms inside the guard bands
//   k_select     one wave per (scan, ring), a lane holds 5 / 6 / 11 consecutive points of a sector in registers: their curvature and the
//                neighbour-gap flags around them are computed from those registers and the next lanes' (curv_window.hpp); the <= 20 edge picks are
//                the head of an independent set that parallel rounds settle (sel_rounds.hpp: winners against the ten neighbours in the
//                lane's and the next lanes' registers, DPP wave shifts), ranked one member per lane; the <= 4 planar picks are repeated
//                64-lane arg-min reductions (DPP) with neighbour suppression; no sort needed;
//                rings longer than the small LDS slice go through a work list to a second launch
//   k_voxel      one workgroup per (scan, ring): voxel-grid down-sampling of the less-flat points (run-length segments from
//                ballots, bucket sort of the segment keys in LDS; <9 slots> / <16 slots> instantiations + work list)
//   k_compact_index  one workgroup per scan: prefix sums over (ring, sector), compaction of the four clouds, line tables, and the (scan line,
//                azimuth bin) index of the two "last" clouds (the steps of line_index.hip) built while their points pass through
// and, outside the registration:
//   k_curvature  one workgroup per 1024-point tile of ONE scan: LDS tile with +-5 halo, the curvature of every point, for the host
//                accessor lmono_batch_get_curvature
// Arithmetic is float/double exactly as the CPU restatement evaluates it (compiled with -ffp-contract=off).
#include "batch.hpp"
#include "curv_window.hpp"
#include "ring_decide.hpp"
#include "sel_rounds.hpp"
#include "vox_runs.hpp"

namespace lmono {

__device__ __forceinline__ int ring_of(float angle, int n_lines, bool &discard)
{
    int id = 0;
    discard = false;
    if (n_lines == 16) {
        id = (int)((double)((angle + 15.0f) / 2.0f) + 0.5);
        if (id > n_lines - 1 || id < 0) discard = true;
    } else if (n_lines == 32) {
        id = (int)(((double)angle + 92.0 / 3.0) * 3.0 / 4.0);
        if (id > n_lines - 1 || id < 0) discard = true;
    } else {
        if ((double)angle >= -8.83)
            id = (int)((double)(2.0f - angle) * 3.0 + 0.5);
        else
            id = n_lines / 2 + (int)((-8.83 - (double)angle) * 2.0 + 0.5);
        if ((double)angle > 2.0 || (double)angle < -24.33 || id > 50 || id < 0) discard = true;
    }
    return id;
}

__device__ __forceinline__ bool point_valid(const float4 &p, float mr2)
{
    return isfinite(p.x) & isfinite(p.y) & isfinite(p.z) & !(p.x * p.x + p.y * p.y + p.z * p.z < mr2);
}

// ------------------------------------------------------------------------------------------------
// Ring sort = stable counting sort of a scan's valid points into ring-major order, as four tile-parallel launches (round 3: one
// workgroup per scan kept ~2 long workgroups per wave slot -- a third of the launch was its tail -- and made one scan alone take 1.1 ms):
//   k_ring_ends     per scan: first / last valid point -> start / end azimuth of the sweep, unit vector of its start direction
//   k_ring_tag      per 4096-point tile: ring id of every point, a [64]-ring histogram per 1024-point wave segment, the first point
//                   past the half sweep, the last valid point
//   k_ring_offsets  per scan: exclusive prefix of the segment histograms in segment order (= input order) per ring, ring_begin
//   k_ring_scatter  per tile: every wave walks its segment in input order with its own running counters (barrier-free multisplit)
// Segment g of scan s lives in row (off[s] >> 10) + s + g of seg_hist: rows of different scans never collide and need no table.
constexpr int kRtT = 256, kRtW = kRtT / 64;    // threads / waves of a tile workgroup
constexpr int kRtSeg = 1024;                   // points per wave segment (4 rounds of 256)
constexpr int kRtTile = kRtSeg * kRtW;

// points of scan s the ring sort looks at: the scan's slot, or the first n_limit of it (one-scan launches of the online stream: the rest of
// the slot is padding)
__device__ __forceinline__ int ring_scan_points(const BatchView &b, int s, int64_t off)
{
    const int n = (int)(b.off[s + 1] - off);
    return b.n_limit > 0 && b.n_limit < n ? b.n_limit : n;
}

__global__ __launch_bounds__(256) void k_ring_ends(BatchView b)
{
    const int s = b.scan0 + blockIdx.x;
    const int64_t off = b.off[s];
    const int n = ring_scan_points(b, s, off);
    const float4 *in = b.in + off;
    const int tid = threadIdx.x, lane = tid & 63;
    __shared__ int s_first;
    if (tid == 0) s_first = INT_MAX;
    __syncthreads();
    const float mr2 = b.min_range * b.min_range;
    // first valid point (it defines the sweep's start azimuth): forward in 256-point chunks until one holds a valid point -- almost always
    // the first.  The LAST valid point is found by k_ring_tag on its way through the scan (the low rings of a 64-line sensor end a scan with
    // thousands of points inside min_range; looking for it from here cost a full read of every scan, 1.9 ms of the round-3 front end).
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid;
        int lf = (i < n && point_valid(in[i], mr2)) ? i : INT_MAX;
        lf = wave_min_i(lf);
        if (lane == 0 && lf != INT_MAX) atomicMin(&s_first, lf);
        __syncthreads();
        const int f = s_first;
        __syncthreads();                   // nobody is in the next chunk's atomicMin before everybody has read this one's result
        if (f != INT_MAX) break;
    }
    if (s_first == INT_MAX) {
        int *rb = b.ring_begin + s * 65;
        if (tid < 65) rb[tid] = 0;
        if (tid == 0) { b.n_cloud[s] = 0; b.scan_ends[s * 2] = -1; b.scan_ends[s * 2 + 1] = -1; b.scan_half[s] = INT_MAX; }
        return;
    }
    if (tid == 0) {
        const float4 p0 = in[s_first];
        b.scan_ori[s * 4] = (float)(-det_atan2((double)p0.y, (double)p0.x));
        float ux, uy;
        ring_start_dir(p0.x, p0.y, ux, uy);
        b.scan_ori[s * 4 + 2] = ux; b.scan_ori[s * 4 + 3] = uy;
        b.scan_ends[s * 2] = s_first; b.scan_ends[s * 2 + 1] = -1;
        b.scan_half[s] = INT_MAX;
    }
}

__global__ __launch_bounds__(kRtT) void k_ring_tag(BatchView b)
{
    const int s = b.scan0 + blockIdx.y;
    const int64_t off = b.off[s];
    const int n = ring_scan_points(b, s, off);
    const int t0 = blockIdx.x * kRtTile;
    if (t0 >= n || b.scan_ends[s * 2] < 0) return;
    const float4 *in = b.in + off;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int s_hist[kRtW][64];
    s_hist[wave][lane] = 0;
    __syncthreads();
    const float mr2 = b.min_range * b.min_range;
    const float startOri = b.scan_ori[s * 4];
    const float ux = b.scan_ori[s * 4 + 2], uy = b.scan_ori[s * 4 + 3];      // start direction (ring_start_dir)
    const int n_lines = b.n_lines;
    const RingMap map = ring_map(n_lines);
    int lh = INT_MAX, ll = -1;
    const int c_lo = t0 + wave * kRtSeg, c_hi = min(c_lo + kRtSeg, n);
    // four points per thread and round, and the NEXT round's four requested before this round's are worked on (unconditional loads, index clamped
    // into the segment): a wave's segment is four rounds, each a load latency + ~450 instructions of angle work -- one behind the other they added up
    float4 nx[4];
#pragma unroll
    for (int q = 0; q < 4; q++) nx[q] = in[min(c_lo + 64 * q + lane, n - 1)];
    for (int r0 = c_lo; r0 < c_hi; r0 += 256) {
        float4 pq[4];
#pragma unroll
        for (int q = 0; q < 4; q++) pq[q] = nx[q];
#pragma unroll
        for (int q = 0; q < 4; q++) nx[q] = in[min(r0 + 256 + 64 * q + lane, n - 1)];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = r0 + 64 * q + lane;
            const float4 p = pq[q];
            int id = -1;
            if ((i < c_hi) & point_valid(p, mr2)) {
                ll = i;                        // i grows with q and r0: the lane's last valid point so far
                // Ring id and the half-sweep test decide between alternatives: ring_decide.hpp settles them without an arctangent (an odd
                // polynomial in z / rho, the signs of a dot and a cross product with the start direction) and without a branch whenever the
                // point is farther than a guard from every threshold; the fp64 forms run only for the points inside a guard band (and for
                // x = y = 0).  The points of a round stay behind one another: with the four fast decisions side by side the compiler paired
                // their float operations (v_pk_mul_f32 / v_pk_add_f32), took 100 registers (4 waves per SIMD) and the pass lost its whole gain.
                const float q2 = p.x * p.x + p.y * p.y;
                bool past_half;
                if (!ring_half_fast(p.x, p.y, p.z, q2, __frsqrt_rn(q2) /* within 1 ulp */, map, ux, uy, id, past_half)) {
                    bool discard;
                    const float angle = (float)(det_atan((double)p.z / sqrt((double)(p.x * p.x + p.y * p.y))) * 180.0 / LM_PI);
                    const int r = ring_of(angle, n_lines, discard);
                    id = -1; past_half = false;
                    if (!discard) {
                        id = r;
                        float o1 = (float)(-det_atan2((double)p.y, (double)p.x));
                        if ((double)o1 < (double)startOri - LM_PI / 2.0) o1 = (float)((double)o1 + 2.0 * LM_PI);
                        else if ((double)o1 > (double)startOri + LM_PI * 3.0 / 2.0) o1 = (float)((double)o1 - 2.0 * LM_PI);
                        past_half = (double)(o1 - startOri) > LM_PI;
                    }
                }
                if (past_half) lh = min(lh, i);
            }
            if (i < c_hi) b.ring_tmp[off + i] = (int8_t)id;
            // histogram of the sub-tile by ballot matching (ring-major input: one or two rings per 64 points)
            unsigned long long rem = __ballot(id >= 0);
            while (rem) {
                const int src = __ffsll((long long)rem) - 1;
                const int k = __shfl(id, src);
                const unsigned long long m = __ballot(id == k);
                if (lane == src) s_hist[wave][k] += __popcll(m);
                rem &= ~m;
            }
        }
    }
    lh = wave_min_i(lh); ll = wave_max_i(ll);
    if (lane == 0 && lh != INT_MAX) atomicMin(&b.scan_half[s], lh);
    if (lane == 0 && ll >= 0) atomicMax(&b.scan_ends[s * 2 + 1], ll);
    __syncthreads();
    if (c_lo < n) b.seg_hist[((size_t)(off >> 10) + (size_t)s + (size_t)(c_lo >> 10)) * 64 + lane] = s_hist[wave][lane];
}

__global__ __launch_bounds__(64) void k_ring_offsets(BatchView b)
{
    const int s = b.scan0 + blockIdx.x;
    if (b.scan_ends[s * 2] < 0) return;
    const int64_t off = b.off[s];
    const int n = ring_scan_points(b, s, off);
    const int nseg = (n + kRtSeg - 1) / kRtSeg, r = threadIdx.x;
    if (r == 0) {                                  // end azimuth of the sweep from the last valid point k_ring_tag found
        const float4 p1 = b.in[off + b.scan_ends[s * 2 + 1]];
        const float startOri = b.scan_ori[s * 4];
        float endOri = (float)((double)(float)(-det_atan2((double)p1.y, (double)p1.x)) + 2.0 * LM_PI);
        if ((double)(endOri - startOri) > 3.0 * LM_PI) endOri = (float)((double)endOri - 2.0 * LM_PI);
        else if ((double)(endOri - startOri) < LM_PI) endOri = (float)((double)endOri + 2.0 * LM_PI);
        b.scan_ori[s * 4 + 1] = endOri;
    }
    int *h = b.seg_hist + ((size_t)(off >> 10) + (size_t)s) * 64 + r;
    int run = 0;
    int g = 0;
    for (; g + 8 <= nseg; g += 8) {              // eight rows in flight per round trip
        int t[8];
#pragma unroll
        for (int u = 0; u < 8; u++) t[u] = h[(size_t)(g + u) * 64];
#pragma unroll
        for (int u = 0; u < 8; u++) { h[(size_t)(g + u) * 64] = run; run += t[u]; }
    }
    for (; g < nseg; g++) { const int t = h[(size_t)g * 64]; h[(size_t)g * 64] = run; run += t; }
    // exclusive scan of the ring totals over the 64 lanes
    int incl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o); if (r >= o) incl += v; }
    int *rb = b.ring_begin + s * 65;
    rb[r] = incl - run;
    if (r == 63) { rb[64] = incl; b.n_cloud[s] = incl; }
}

__global__ __launch_bounds__(kRtT) void k_ring_scatter(BatchView b)
{
    const int s = b.scan0 + blockIdx.y;
    const int64_t off = b.off[s];
    const int n = ring_scan_points(b, s, off);
    const int t0 = blockIdx.x * kRtTile;
    if (t0 >= n || b.scan_ends[s * 2] < 0) return;
    const float4 *in = b.in + off;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int s_pos[kRtW][64];            // next output position of (wave, ring)
    __shared__ double s_atan[17];              // kAtanTab in LDS: the azimuth of every kept point looks it up per lane
    if (tid < 17) s_atan[tid] = kAtanTab[tid];
    const int c_lo = t0 + wave * kRtSeg, c_hi = min(c_lo + kRtSeg, n);
    s_pos[wave][lane] = c_lo < n ? b.seg_hist[((size_t)(off >> 10) + (size_t)s + (size_t)(c_lo >> 10)) * 64 + lane] + b.ring_begin[s * 65 + lane] : 0;
    __syncthreads();
    const float startOri = b.scan_ori[s * 4], endOri = b.scan_ori[s * 4 + 1];
    const int half = b.scan_half[s];
    for (int r0 = c_lo; r0 < c_hi; r0 += 256) {
        int id[4], dstp[4];
        // unconditional loads (index clamped into the segment): behind their guards the four byte loads were waited for one by one
        signed char idb[4];
#pragma unroll
        for (int q = 0; q < 4; q++) { const int i = r0 + 64 * q + lane; idb[q] = b.ring_tmp[off + min(i, c_hi - 1)]; }
#pragma unroll
        for (int q = 0; q < 4; q++) { const int i = r0 + 64 * q + lane; id[q] = (i < c_hi) ? (int)idb[q] : -1; }
        float4 pq[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = r0 + 64 * q + lane;
            pq[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (id[q] >= 0) pq[q] = in[i];
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            dstp[q] = 0;
            unsigned long long rem = __ballot(id[q] >= 0);
            while (rem) {
                const int src = __ffsll((long long)rem) - 1;
                const int k = __shfl(id[q], src);
                const unsigned long long m = __ballot(id[q] == k);
                int base = 0;
                if (lane == src) { base = s_pos[wave][k]; s_pos[wave][k] = base + __popcll(m); }
                base = __shfl(base, src);
                if (id[q] == k) dstp[q] = base + __popcll(m & ((1ull << lane) - 1ull));
                rem &= ~m;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = r0 + 64 * q + lane;
            if (id[q] >= 0) {
                const float4 p = pq[q];
                float ori = (float)(-det_atan2((double)p.y, (double)p.x, s_atan));      // the azimuth itself is a result (relTime): always the fp64 form
                if (i <= half) {
                    if ((double)ori < (double)startOri - LM_PI / 2.0) ori = (float)((double)ori + 2.0 * LM_PI);
                    else if ((double)ori > (double)startOri + LM_PI * 3.0 / 2.0) ori = (float)((double)ori - 2.0 * LM_PI);
                } else {
                    ori = (float)((double)ori + 2.0 * LM_PI);
                    if ((double)ori < (double)endOri - LM_PI * 3.0 / 2.0) ori = (float)((double)ori + 2.0 * LM_PI);
                    else if ((double)ori > (double)endOri + LM_PI / 2.0) ori = (float)((double)ori - 2.0 * LM_PI);
                }
                const float relTime = (ori - startOri) / (endOri - startOri);
                const float inten = (float)((double)id[q] + 0.1 * (double)relTime);
                b.cloud[off + dstp[q]] = make_float4(p.x, p.y, p.z, inten);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_curvature: the curvature of every point of ONE scan's ring-sorted cloud, for the host accessor (lmono_batch_get_curvature).  The
// registration does not run it: k_select computes the curvature and the gap flags of a sector from the cloud (curv_window.hpp).
constexpr int kCurvTile = 1024;

__global__ __launch_bounds__(256) void k_curvature(BatchView b, int s, float *curv)
{
    const int n = b.n_cloud[s];
    const int t0 = blockIdx.x * kCurvTile;
    if (t0 >= n) return;
    const int64_t off = b.off[s];
    const float4 *c = b.cloud + off;
    __shared__ float sx[kCurvTile + 10], sy[kCurvTile + 10], sz[kCurvTile + 10];
    for (int k = threadIdx.x; k < kCurvTile + 10; k += 256) {
        const int i = t0 - 5 + k;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i >= 0 && i < n) p = c[i];
        sx[k] = p.x; sy[k] = p.y; sz[k] = p.z;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kCurvTile; k += 256) {
        const int i = t0 + k;
        if (i >= n) break;
        const int q = k + 5;
        float cv = 0.f;
        if (i >= 5 && i < n - 5) {
            const float dx = sx[q - 5] + sx[q - 4] + sx[q - 3] + sx[q - 2] + sx[q - 1] - 10 * sx[q] + sx[q + 1] + sx[q + 2] + sx[q + 3] + sx[q + 4] + sx[q + 5];
            const float dy = sy[q - 5] + sy[q - 4] + sy[q - 3] + sy[q - 2] + sy[q - 1] - 10 * sy[q] + sy[q + 1] + sy[q + 2] + sy[q + 3] + sy[q + 4] + sy[q + 5];
            const float dz = sz[q - 5] + sz[q - 4] + sz[q - 3] + sz[q - 2] + sz[q - 1] - 10 * sz[q] + sz[q + 1] + sz[q + 2] + sz[q + 3] + sz[q + 4] + sz[q + 5];
            cv = dx * dx + dy * dy + dz * dz;
        }
        curv[i] = cv;
    }
}

// ------------------------------------------------------------------------------------------------
// k_select: one WAVE per (scan, ring); 4 rings per 256-thread workgroup, no workgroup barriers.
// The reference sorts every sector by curvature and walks the sorted order taking the next un-suppressed point
// (<= 20 largest with c > 0.1, then <= 4 smallest with c < 0.1).  Walking a sorted order and repeatedly taking the
// extremum of the not-yet-suppressed points visit the same points in the same order, so no sort is needed: each lane
// keeps its sector elements (curvature, suppressed flag) in registers and a pick is one 64-lane arg-max / arg-min
// over the packed key (curvature bits, index), which also reproduces the (curvature, index) tie order of the sort.
// The flat picks run exactly so.  The sharp picks do not take 21 reductions one after the other: the points that such a
// walk takes are the 20 of highest key of an independent set that parallel rounds find (sel_rounds.hpp, two rounds for
// most sectors), and they are ranked one per lane afterwards.
// The curvature is not read from memory: a sector's elements and their ten neighbours are the registers of the lane and of the two lanes
// next to it, so the wave computes curvature and gap flags of the sector from the ring-sorted cloud itself (curv_window.hpp), with
// k_curvature's operands in k_curvature's order.  Sector elements lie in ring-local [5, len - 6]: every neighbour is in the same ring.
constexpr int kSelMaxPerLane = (kRingCap / 6 + 1 + 63) / 64;   // 11 elements per lane for the largest legal sector

// key of a sector element: hi = curvature bits, lo = (index << 8 | suppression reach).  Ordering by (hi, lo) = ordering by
// (curvature, index), so the arg-max / arg-min over keys reproduces the sort's tie order; the winner's reach rides along.
// A pick is ONE 32-bit wave reduction: the curvature decides; the winner's low word is read from its lane when a single lane holds the
// extremum (the rule: equal curvatures in two lanes are rare), a second reduction over the low words settles the ties otherwise.
__device__ __forceinline__ unsigned int select_lo(int idx, unsigned int reach) { return ((unsigned int)idx << 8) | reach; }

// whole-wave shifts by one lane (DPP wave_shr:1 / wave_shl:1): the value of the lane before / behind; 0 where the wave ends (bound_ctrl)
__device__ __forceinline__ unsigned int lane_before(unsigned int v) { return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true); }
__device__ __forceinline__ unsigned int lane_behind(unsigned int v) { return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, true); }

// one sector of one ring, M consecutive elements per lane (element m of a lane is ring-local index sp + lane M + m): the ten
// neighbours that a round of the sharp picks compares an element with are registers of the lane or of the two lanes next to it
constexpr int kSelScratch = 64 * 8;      // per wave: one (curvature bits, index | reach) pair per lane, the members of a sector for ranking

// the lanes of curv_window.hpp: the shifts above with bound_ctrl off, so that the lane at the wave's end keeps `old`
struct SelLanes {
    typedef unsigned int bits;
    __device__ __forceinline__ unsigned int before(unsigned int v, unsigned int old) const { return (unsigned int)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x138, 0xf, 0xf, false); }
    __device__ __forceinline__ unsigned int behind(unsigned int v, unsigned int old) const { return (unsigned int)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x130, 0xf, 0xf, false); }
    __device__ __forceinline__ float before(float v, float old) const { return __uint_as_float(before(__float_as_uint(v), __float_as_uint(old))); }
    __device__ __forceinline__ float behind(float v, float old) const { return __uint_as_float(behind(__float_as_uint(v), __float_as_uint(old))); }
};

template <int M>
__device__ __forceinline__ void select_sector(int lane, int j, int sp, int slen, int rbeg, const float4 *pts, unsigned char *picked,
                                              signed char *label, int *sel_sh, int *sel_sh_n, int *sel_fl, int *sel_fl_n,
                                              unsigned int *scratch)
{
    unsigned int kh[M], kl[M];
    unsigned int dead = 0, big = 0, small = 0;     // bit m: suppressed / out of range; curvature > 0.1; < 0.1
    // (the lane as a value of this sector's own: what derives from it -- lane M + m, the ballot masks, the halo's side -- is then a few
    // instructions per sector, where the compiler otherwise computes all of it once per ring for the three instantiations and keeps it
    // in scratch)
    asm volatile("" : "+v"(lane));
    const int e0 = lane * M;
    // The curvature of the lane's elements and the gap flags around them, from the ring's points (pts = the ring's first; curv_window.hpp).
    // Element e of the sector is ring point sp + e, and its windows read the points sp - 5 .. ep + 5 = sp + slen + 4, all of them in the
    // ring (sp >= 5, ep <= len - 6).  A lane loads its M points whether they are elements or not: the lanes behind the sector's end hold
    // the points that follow it, which is the halo of the last elements, and read point ep + 5 again where they would go further (what
    // they compute is used by nobody).  Lane 0 fetches the five points before the sector, lane 63 the five behind its own.
    // gwin: bit k = gap flag of point sp + e0 - 5 + k, k < M + 9.
    float cv[M];
    unsigned int gwin;
    {
        // (every lane behind lane 0 loads lane 63's halo, one address for 63 lanes: cheaper than a branch around the loads)
        const int last = slen + 4;
        const float4 *hp = pts + sp + (lane == 0 ? -kCurvReach : min(64 * M, last));
        const int hmax = lane == 0 ? kCurvReach : max(last - 64 * M, 0);       // halo point d stands at hp[min(d, hmax)]
        const SelLanes lanes;
        unsigned int hb;
        float hx0, hy0, hz0;
        {
            float h[3][kCurvReach + 1];
#pragma unroll
            for (int d = 0; d <= kCurvReach; d++) {
                const float4 p = hp[min(d, hmax)];          // lane 0's sixth: the sector's first point
                h[0][d] = p.x; h[1][d] = p.y; h[2][d] = p.z;
            }
            hb = curv_halo_flags<unsigned int>(h[0], h[1], h[2]);
            hx0 = h[0][0]; hy0 = h[1][0]; hz0 = h[2][0];
        }
        float o[3][M];
#pragma unroll
        for (int m = 0; m < M; m++) {
            const float4 p = pts[sp + min(e0 + m, last)];
            o[0][m] = p.x; o[1][m] = p.y; o[2][m] = p.z;
        }
        gwin = curv_gap_window<M>(lanes, o[0], o[1], o[2], hx0, hy0, hz0, hb);
        // (the halo again, one coordinate at a time: fifteen registers through the three passes cost more than these loads)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float h[kCurvReach];
#pragma unroll
            for (int d = 0; d < kCurvReach; d++) h[d] = ((const float *)(hp + min(d, hmax)))[c];
            if constexpr (M <= 6) {
                curv_window_coord<M>(lanes, o[c], h, c == 0, cv);
            } else {
                // the wide instantiation has no registers for 33 coordinates beside a window of 21: it fetches its points again
                // (through an index the compiler cannot see through, or it keeps the first fetch's registers after all)
                float oc[M];
                int ec = e0;
                asm volatile("" : "+v"(ec));
#pragma unroll
                for (int m = 0; m < M; m++) oc[m] = ((const float *)(pts + sp + min(ec + m, last)))[c];
                curv_window_coord<M>(lanes, oc, h, c == 0, cv);
            }
        }
    }
    // (double)c > 0.1 and (double)c < 0.1 as float compares: 0.1f is the smallest float above the double 0.1, so c > 0.1 iff c >= 0.1f and
    // c < 0.1 iff c < 0.1f, for every float c (a NaN fails both either way)
#pragma unroll
    for (int m = 0; m < M; m++) {
        const int e = e0 + m;
        const bool in = e < slen;
        const int i = sp + min(e, slen - 1);
        const float c = cv[m];
        // suppression reach: the neighbour walk marks l = 1..5 forward while the gap before point i+l is short, and the same backward --
        // the zero runs above / below bit i of the ring's gap BIT mask
        const unsigned int win = gwin >> m;                                                       // bit k = gap flag of point i - 5 + k
        const int lf = min(5, __ffs((int)((win >> 5) | 32u)) - 1);
        const int lb = min(5, __clz((int)((win & 31u) << 27)));
        kh[m] = in ? __float_as_uint(c) : 0u; kl[m] = in ? select_lo(i, (unsigned int)(lf | (lb << 4))) : 0u;
        dead |= (unsigned int)(!in | (picked[i] != 0)) << m;
        big |= (unsigned int)(in & (c >= 0.1f)) << m;
        small |= (unsigned int)(in & (c < 0.1f)) << m;
    }
    // ---- largest curvature first: <= 2 sharp, <= 20 less sharp
    // The picks are the 20 members of highest key of the lexicographically first independent set of the live candidates (sel_rounds.hpp),
    // which parallel rounds settle: winners join, what lies within a winner's reach dies, until nothing is live -- two rounds for most
    // sectors, one per step for a staircase of curvatures.
    int largest = 0;
    unsigned int members = 0u;
    {
        unsigned int live = big & ~dead;
        while (__ballot(live != 0u)) {
            unsigned int x[M + 2 * kSelReach];
#pragma unroll
            for (int m = 0; m < M; m++) x[m + kSelReach] = kh[m] & (unsigned int)((int)(live << (31 - m)) >> 31);
#pragma unroll
            for (int d = 0; d < kSelReach; d++) {
                x[d] = lane_before(x[M + d]);                            // element M - 5 + d of the lane before
                x[M + kSelReach + d] = lane_behind(x[kSelReach + d]);     // element d of the lane behind
            }
            const unsigned int w = sel_winners<M>(x, gwin);
            members |= w;
            live &= ~sel_deaths<M>(sel_window<M>(lane_before(w), w, lane_behind(w)), gwin);
        }
    }
    int n_mem = 0;
#pragma unroll
    for (int m = 0; m < M; m++) n_mem += __popcll(__ballot((members >> m) & 1u));
    // More than 64 members (15 % of the sectors of the headline world, 80 % of the cluttered one: profiles/r17/NOTES.md): the members below the 20th largest of the lanes' best curvatures
    // cannot be among the 20 picks (sel_rounds.hpp) and are left out of the ranking.
    unsigned int top = members;
    if (n_mem > 64) {
        const unsigned int best = sel_lane_best<M>(members, kh);
        int above = 0;
        for (int t = 0; t < 64; t++) above += (unsigned int)__builtin_amdgcn_readlane((int)best, t) > best ? 1 : 0;
        top = sel_keep_from<M>(members, kh, wave_min_u32_uniform(above < kSelSharpMax ? best : ~0u));
    }
    // the members to rank one per lane (ballot ranks, through 512 B of LDS)
    int n_top = 0;
#pragma unroll
    for (int m = 0; m < M; m++) {
        const bool is = (top >> m) & 1u;
        const unsigned long long mk = __ballot(is);
        const int pos = n_top + __popcll(mk & ((1ull << lane) - 1ull));
        if (is && pos < 64) { scratch[2 * pos] = kh[m]; scratch[2 * pos + 1] = kl[m]; }
        n_top += __popcll(mk);
    }
    const bool ranked = n_top <= 64;
    if (ranked) {
        __builtin_amdgcn_wave_barrier();           // one wave: its LDS operations execute in order; the barrier keeps the compiler from reordering them
        unsigned int ch = 0u, cl = 0u;
        if (lane < n_top) { ch = scratch[2 * lane]; cl = scratch[2 * lane + 1]; }
        __builtin_amdgcn_wave_barrier();           // the next sector's writes stay behind these reads
        // rank = members of a larger key; the 20 first are the picks, and only they leave marks
        int rank = 0;
        for (int t = 0; t < n_top; t++) {
            const unsigned int th = (unsigned int)__builtin_amdgcn_readlane((int)ch, t), tl = (unsigned int)__builtin_amdgcn_readlane((int)cl, t);
            rank += sel_key_above(th, tl, ch, cl) ? 1 : 0;
        }
        if (lane < n_top && rank < kSelSharpMax) {
            const int pind = (int)(cl >> 8), lf = sel_lf(cl), lb = sel_lb(cl);
            sel_sh[j * 20 + rank] = rbeg + pind; label[pind] = rank < 2 ? 2 : 1;
#pragma unroll
            for (int o = 0; o <= 2 * kSelReach; o++) picked[pind - lb + min(o, lf + lb)] = 1;      // (a short reach writes its last byte again)
        }
        largest = n_mem;
        __builtin_amdgcn_wave_barrier();
        // what the picks suppressed, for the flat picks: the picked bytes of the lane's elements
#pragma unroll
        for (int m = 0; m < M; m++) dead |= (unsigned int)(picked[sp + min(e0 + m, slen - 1)] != 0) << m;     // (behind the end: dead already)
    }
    // more than 64 left to rank (equal curvatures in more than 64 members, or members in fewer than 20 lanes): one pick after the other, the
    // wave-wide arg-max of what is live.  The walk starts again from the `dead` of the load: what the rounds, the bound and the compaction
    // found is not used (a rare path; nothing has been written to `picked`, the labels or `sel_sharp` yet).
    while (!ranked) {
        const unsigned int live = big & ~dead;
        // the lane's own best: slots ascend in index, so ">=" keeps the larger index among equal curvatures (live curvatures are > 0.1: 0 = none)
        unsigned int bh = 0u, bl = 0u;
#pragma unroll
        for (int m = 0; m < M; m++) {
            const unsigned int h = kh[m] & (unsigned int)((int)(live << (31 - m)) >> 31);
            const bool t = h >= bh;
            bh = t ? h : bh; bl = t ? kl[m] : bl;
        }
        const unsigned int mh = wave_max_u32_uniform(bh);
        if (mh == 0u) break;
        const unsigned long long who = __ballot(bh == mh);
        unsigned int lo;
        if ((who & (who - 1ull)) == 0ull) lo = (unsigned int)__builtin_amdgcn_readlane((int)bl, __ffsll((long long)who) - 1);
        else lo = wave_max_u32_uniform(bh == mh ? bl : 0u);
        const int pind = (int)(lo >> 8), lf = (int)(lo & 15u), lb = (int)((lo >> 4) & 15u);
        largest++;
        if (largest > 20) break;
        if (lane == 0) { sel_sh[j * 20 + largest - 1] = rbeg + pind; label[pind] = largest <= 2 ? 2 : 1; }
        if (lane <= lf + lb) picked[pind - lb + lane] = 1;
        dead |= sel_hit_bits<M>(pind - lb - sp - e0, lb + lf);      // the lane's elements inside the suppressed range [pind - lb, pind + lf]
    }
    if (lane == 0) sel_sh_n[j] = largest > 20 ? 20 : largest;
    // ---- smallest curvature first: <= 4 flat
    int smallest = 0;
    while (true) {
        const unsigned int live = small & ~dead;
        // "<" keeps the smaller index among equal curvatures; a dead slot reads as ~0 (a live curvature is < 0.1)
        unsigned int bh = ~0u, bl = ~0u;
#pragma unroll
        for (int m = 0; m < M; m++) {
            const unsigned int h = kh[m] | ~(unsigned int)((int)(live << (31 - m)) >> 31);
            const bool t = h < bh;
            bh = t ? h : bh; bl = t ? kl[m] : bl;
        }
        const unsigned int mh = wave_min_u32_uniform(bh);
        if (mh == ~0u) break;
        const unsigned long long who = __ballot(bh == mh);
        unsigned int lo;
        if ((who & (who - 1ull)) == 0ull) lo = (unsigned int)__builtin_amdgcn_readlane((int)bl, __ffsll((long long)who) - 1);
        else lo = wave_min_u32_uniform(bh == mh ? bl : ~0u);
        const int pind = (int)(lo >> 8), lf = (int)(lo & 15u), lb = (int)((lo >> 4) & 15u);
        if (lane == 0) { label[pind] = -1; sel_fl[j * 4 + smallest] = rbeg + pind; }
        smallest++;
        if (smallest >= 4) break;
        if (lane <= lf + lb) picked[pind - lb + lane] = 1;
        dead |= sel_hit_bits<M>(pind - lb - sp - e0, lb + lf);      // the lane's elements inside the suppressed range [pind - lb, pind + lf]
    }
    if (lane == 0) sel_fl_n[j] = smallest;
}

// The 11-element instantiation (rings of the second launch) as a function of its own: its registers and spills stay out of the code
// of the 5- and 6-element sectors that every HDL-64 ring runs.
__device__ __noinline__ void select_sector_wide(int lane, int j, int sp, int slen, int rbeg, const float4 *pts, unsigned char *picked,
                                                signed char *label, int *sel_sh, int *sel_sh_n, int *sel_fl, int *sel_fl_n,
                                                unsigned int *scratch)
{
    select_sector<kSelMaxPerLane>(lane, j, sp, slen, rbeg, pts, picked, label, sel_sh, sel_sh_n, sel_fl, sel_fl_n, scratch);
}

// wave-uniform values as scalars (the compiler cannot prove uniformity of what is loaded through a per-wave index)
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long uni64(long long v)
{
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)v), hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
// (through address space 1: the integer round trip would otherwise leave a generic pointer and flat_ loads / stores behind)
template <typename T> __device__ __forceinline__ T *uni_ptr(T *p)
{
    typedef __attribute__((address_space(1))) T GT;
    return (T *)(GT *)uni64((long long)p);
}

// LDS slice of one wave for rings of up to `cap` points: picked bytes (the second half held the ring's gap bit mask and is not used)
__host__ __device__ constexpr int sel_slice_bytes(int cap) { return 2 * cap; }

// one ring by one wave; cap = ring points the wave's LDS slice (sel_slice_bytes(cap) at smem_w) can hold
__device__ __forceinline__ void select_ring(BatchView &b, int r, int s, int lane, unsigned char *smem_w, int cap, bool may_defer, unsigned int *scratch)
{
    r = uni(r); s = uni(s);
    const int64_t off = uni64(b.off[s]);
    const int *rb = b.ring_begin + s * 65;
    const int rbeg = uni(rb[r]), rend = uni(rb[r + 1]), len = rend - rbeg;
    const int S = rbeg + 5, E = rend - 6;
    int *sel_sh = uni_ptr(b.sel_sharp + (size_t)((s * 64 + r) * kSectors) * 20);
    int *sel_sh_n = uni_ptr(b.sel_sharp_n + (s * 64 + r) * kSectors);
    int *sel_fl = uni_ptr(b.sel_flat + (size_t)((s * 64 + r) * kSectors) * 4);
    int *sel_fl_n = uni_ptr(b.sel_flat_n + (s * 64 + r) * kSectors);
    if (E - S < 6 || len > kRingCap) {
        if (lane < kSectors) { sel_sh_n[lane] = 0; sel_fl_n[lane] = 0; }
        if (lane == 0 && len > kRingCap) atomicOr(&b.status[s], kStatusRingOverflow);
        for (int i = lane; i < len; i += 64) b.label[off + rbeg + i] = 0;
        return;
    }
    if (len > cap) {
        // longer than this launch's LDS slice: left to the second launch (full-size slices, small grid over the work list)
        if (may_defer && lane == 0) b.sel_todo[1 + atomicAdd(&b.sel_todo[0], 1)] = (s << 6) | r;
        return;
    }
    // labels go straight to HBM (zeroed here, ~144 single-byte stores per ring afterwards): the LDS slice only holds the
    // picked bytes
    unsigned char *picked = smem_w;
    signed char *label = uni_ptr((signed char *)(b.label + off + rbeg));
    const float4 *pts = uni_ptr((const float4 *)(b.cloud + off + rbeg));
    const int span = E - S;
#pragma unroll 1
    for (int i = lane; i < len; i += 64) { picked[i] = 0; label[i] = 0; }
    __builtin_amdgcn_wave_barrier();
    for (int j = 0; j < kSectors; j++) {
        const int sp = 5 + span * j / 6;
        const int ep = 5 + span * (j + 1) / 6 - 1;
        const int slen = ep - sp + 1;
        // HDL-64-sized sectors (<= 320 / <= 384 points) take the 5- / 6-slot instantiations, longer rings the full one
        if (slen <= 5 * 64) select_sector<5>(lane, j, sp, slen, rbeg, pts, picked, label, sel_sh, sel_sh_n, sel_fl, sel_fl_n, scratch);
        else if (slen <= 6 * 64) select_sector<6>(lane, j, sp, slen, rbeg, pts, picked, label, sel_sh, sel_sh_n, sel_fl, sel_fl_n, scratch);
        else select_sector_wide(lane, j, sp, slen, rbeg, pts, picked, label, sel_sh, sel_sh_n, sel_fl, sel_fl_n, scratch);
    }
}

// Two launches: the first gives every wave a slice for kSelSmallCap points (every HDL-64 ring; 18 KB per workgroup instead of
// 32 KB) over the whole (ring, scan) grid and defers longer rings to a work list; the second
// runs full-size slices as a small fixed grid over that list (normally empty).
constexpr int kSelSmallCap = 2304, kSelBigGrid = 128;

__global__ __launch_bounds__(256, 8) void k_select(BatchView b, int cap, int from_list)
{
    // the wave index as a scalar: ring, scan, the ring's bounds and every output pointer derived from it stay in SGPRs (as VGPRs they
    // pushed the 64-register budget of 8 waves / SIMD over and the pick loop reloaded a spilled pointer on every pick)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char *smem_w = smem + wave * sel_slice_bytes(cap);
    unsigned int *scratch = (unsigned int *)(smem + 4 * sel_slice_bytes(cap) + wave * kSelScratch);      // behind the four slices (a slice is a multiple of 8 bytes)
    if (!from_list) {
        select_ring(b, blockIdx.x * 4 + wave, b.scan0 + blockIdx.y, lane, smem_w, cap, true, scratch);
    } else {
        const int n_todo = b.sel_todo[0];
        for (int k = blockIdx.x * 4 + wave; k < n_todo; k += gridDim.x * 4) {
            const int e = b.sel_todo[1 + k];
            select_ring(b, e & 63, e >> 6, lane, smem_w, cap, false, scratch);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_voxel: one workgroup per (scan, ring): pcl::VoxelGrid(0.2 m, all fields averaged) over the ring's less-flat
// candidates (label <= 0 inside the sectors).  PCL sorts (cell, point) pairs and averages each cell's points in that
// order.  Consecutive ring points mostly share a voxel, so the points are first run-length compressed into segments
// (cell, first index); only the segments are sorted and a voxel's centroid is the float sum over its segments in
// (cell, first index) order = (cell, point index) order.
//
// Layout: point i = tid + 256 m of the ring sits in register slot m of thread tid, so wave w of slot m holds 64
// consecutive points and a ballot over the wave is a 64-bit piece of a per-ring bitmap (word i >> 6).  Segment heads,
// their count and their positions come from ballots and a prefix over (slot, wave); "point i continues the run
// of point i - 1" is kept as a bitmap, which is all the accumulation needs to know about run lengths: a run's length is a count
// of trailing ones in a window of two of its words (vox_runs.hpp).
// Sort: a bucket sort -- bucket = cell index shifted down to <= 2048 / 4096 values (monotone in the cell), histogram ->
// exclusive prefix -> cursors, keys scattered bucket by bucket in arrival order, then every key counts the smaller keys of its
// bucket and takes that place: the exact (cell, first index) order whatever the arrival order was.  A key mostly has 1-3
// companions in its bucket, but a wave of 64 keys runs as long as its largest bucket, ~18 keys on an HDL-64 ring (a bucket spans
// a few rows of x, and where the ring runs along x dozens of segments share one), so the small instantiation makes a trip one
// LDS read of a one-word key and two compares, and finds the voxel starts in the same loop.  Rings the bucket sort does not
// take fall back to the register bitonic network.
// Accumulation: one voxel per thread and round; its segments are [vstart[v], vstart[v + 1]) of the sorted array, which holds
// the first indices, so a segment costs one LDS read, the window and the loads of its points.
//
// Two instantiations run back to back: <9 slots, 2048 buckets> takes the rings of <= 2304 points and <= 2^31 cells (every HDL-64
// ring: 68 VGPRs, 24.5 KB of LDS, 6 workgroups per CU) and appends a ring it cannot take to a work list; <16 slots, 4096 buckets>
// runs as a small fixed grid over that list (normally empty): bucket sort up to 1024 segments and 2^32 cells, bitonic network beyond.
constexpr int kVoxBucketSegsBig = 1024;   // bucket-sort capacity (segments) of the big instantiation; the small one takes its whole ring
constexpr int kVoxSmallSlots = 9, kVoxSmallBits = 11;
constexpr int kVoxBigSlots = kRingCap / 256, kVoxBigBits = 12;
constexpr int kVoxBigGrid = 512;    // workgroups of the second instantiation; each walks the work list with this stride
// LDS: key region (sorted keys | scattered copy | bucket counters; the big variant: kRingCap keys for the bitonic fallback),
// 256 scratch ints, the continuation bitmap and the last cells
template <int kSlots, int kBits, bool kSmall>
struct VoxCfg {
    static constexpr int kSegCap = kSmall ? 256 * kSlots : kVoxBucketSegsBig;
    // small: scattered keys as (cell bits below the bucket << 12 | first index, u32) and their buckets (u16) | sorted segments as
    // (voxel start << 15 | first index, u16) | bucket counters (u16, two per word), later the voxel starts (u16)
    static constexpr int kHistBytes = (1 << kBits) * 2 > kSegCap * 2 ? (1 << kBits) * 2 : kSegCap * 2;
    static constexpr int kKeyBytes = kSmall ? kSegCap * 4 + kSegCap * 2 + kSegCap * 2 + kHistBytes : kRingCap * 8;
    // the continuation bitmap ends in two zero words (vox_runs.hpp)
    static constexpr int kLds = kKeyBytes + 1024 + (kSlots * 4 + 2) * 8 + kSlots * 4 * 4;
};
static_assert(256 * kVoxSmallSlots <= 4096, "a first index of the small instantiation has 12 bits");
static_assert((1 << kVoxSmallBits) == 2048, "the small instantiation's counters are one uint4 per thread");
constexpr int kVoxLdsSmall = VoxCfg<kVoxSmallSlots, kVoxSmallBits, true>::kLds;
constexpr int kVoxLdsBig = VoxCfg<kVoxBigSlots, kVoxBigBits, false>::kLds;
static_assert(2 * kVoxBucketSegsBig * 8 + (1 << kVoxBigBits) * 4 <= kRingCap * 8, "bucket sort scratch must fit the key region");
#ifdef LMONO_VOX_PROF
#define VT(i) { if (blockIdx.x == 20 && blockIdx.y == 3 && threadIdx.x == 0) vt[i] = clock64(); }
#else
#define VT(i)
#endif

// min / max over the wave with a wave-uniform result: the DPP stages of common.hpp's wave_min_u32_uniform (one VALU instruction each,
// no LDS crossbar); a lane without a source takes the identity.  No input is a NaN here, so the order of the stages does not matter.
template <int kCtrl, int kRowMask>
__device__ __forceinline__ float dpp_mov_f32(float v, float ident)
{
    return __uint_as_float(dpp_mov_u32<kCtrl, kRowMask>(__float_as_uint(v), __float_as_uint(ident)));
}
__device__ __forceinline__ float wave_min_f(float v)
{
    v = fminf(v, dpp_mov_f32<0x111, 0xf>(v, FLT_MAX));
    v = fminf(v, dpp_mov_f32<0x112, 0xf>(v, FLT_MAX));
    v = fminf(v, dpp_mov_f32<0x114, 0xf>(v, FLT_MAX));
    v = fminf(v, dpp_mov_f32<0x118, 0xf>(v, FLT_MAX));
    v = fminf(v, dpp_mov_f32<0x142, 0xa>(v, FLT_MAX));
    v = fminf(v, dpp_mov_f32<0x143, 0xc>(v, FLT_MAX));
    return __uint_as_float((unsigned int)__builtin_amdgcn_readlane((int)__float_as_uint(v), 63));
}
__device__ __forceinline__ float wave_max_f(float v)
{
    v = fmaxf(v, dpp_mov_f32<0x111, 0xf>(v, -FLT_MAX));
    v = fmaxf(v, dpp_mov_f32<0x112, 0xf>(v, -FLT_MAX));
    v = fmaxf(v, dpp_mov_f32<0x114, 0xf>(v, -FLT_MAX));
    v = fmaxf(v, dpp_mov_f32<0x118, 0xf>(v, -FLT_MAX));
    v = fmaxf(v, dpp_mov_f32<0x142, 0xa>(v, -FLT_MAX));
    v = fmaxf(v, dpp_mov_f32<0x143, 0xc>(v, -FLT_MAX));
    return __uint_as_float((unsigned int)__builtin_amdgcn_readlane((int)__float_as_uint(v), 63));
}
// inclusive prefix sum across the wave in six DPP stages (the row_shr / row_bcast ladder of the reductions above, which leaves every
// lane with the sum of the lanes up to it); a lane without a source adds 0
__device__ __forceinline__ int wave_scan_incl_dpp(int v)
{
    v += (int)dpp_mov_u32<0x111, 0xf>((unsigned int)v, 0u);
    v += (int)dpp_mov_u32<0x112, 0xf>((unsigned int)v, 0u);
    v += (int)dpp_mov_u32<0x114, 0xf>((unsigned int)v, 0u);
    v += (int)dpp_mov_u32<0x118, 0xf>((unsigned int)v, 0u);
    v += (int)dpp_mov_u32<0x142, 0xa>((unsigned int)v, 0u);
    v += (int)dpp_mov_u32<0x143, 0xc>((unsigned int)v, 0u);
    return v;
}

template <int kVoxSlots, int kVoxBucketBits, bool kSmall>
__device__ __forceinline__ void voxel_ring(BatchView &b, int r, int s);

template <int kVoxSlots, int kVoxBucketBits, bool kSmall>
__global__ __launch_bounds__(256) void k_voxel(BatchView b)
{
    if (kSmall) voxel_ring<kVoxSlots, kVoxBucketBits, kSmall>(b, blockIdx.x, b.scan0 + blockIdx.y);
    else {
        const int n_todo = b.vox_todo[0];
        for (int k = blockIdx.x; k < n_todo; k += gridDim.x) {
            const int e = b.vox_todo[1 + k];
            voxel_ring<kVoxSlots, kVoxBucketBits, kSmall>(b, e & 63, e >> 6);
            __syncthreads();
        }
    }
}

template <int kVoxSlots, int kVoxBucketBits, bool kSmall>
__device__ __forceinline__ void voxel_ring(BatchView &b, int r, int s)
{
    constexpr int kVoxBuckets = 1 << kVoxBucketBits;
    constexpr int kCap = 256 * kVoxSlots;
    constexpr int kKeyBytes = VoxCfg<kVoxSlots, kVoxBucketBits, kSmall>::kKeyBytes;
    constexpr int kVoxBucketSegs = VoxCfg<kVoxSlots, kVoxBucketBits, kSmall>::kSegCap;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t off = b.off[s];
#ifdef LMONO_VOX_PROF
    long long vt[8];
#endif
    VT(0)
    const int *rb = b.ring_begin + s * 65;
    const int rbeg = rb[r], rend = rb[r + 1], len = rend - rbeg;
    const int S = rbeg + 5, E = rend - 6;
    if (kSmall && len > kCap && len <= kRingCap && E - S >= 6) {
        if (tid == 0) b.vox_todo[1 + atomicAdd(&b.vox_todo[0], 1)] = (s << 6) | r;    // the big instantiation's ring
        return;
    }
    if (E - S < 6 || len > kRingCap) {
        if (tid == 0) b.lf_n[s * 64 + r] = 0;
        return;
    }
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long *keys = (unsigned long long *)smem;                  // sorted segment keys (cell << 32 | first index)
    int *scr = (int *)(smem + kKeyBytes);                                   // 256 ints
    unsigned long long *contw = (unsigned long long *)(smem + kKeyBytes + 1024);   // [kVoxSlots * 4 + 2] run-continuation bitmap, two zero words behind it
    unsigned int *lastc = (unsigned int *)(contw + kVoxSlots * 4 + 2);      // [kVoxSlots * 4] cell of lane 63 of every (slot, wave)
    const signed char *label = (const signed char *)(b.label + off + rbeg);
    const float4 *cl = b.cloud + off + rbeg;
    const int c_lo = 5, c_hi = len - 7;   // sectors cover local [5, len-7]
    float mnx = FLT_MAX, mny = FLT_MAX, mnz = FLT_MAX, mxx = -FLT_MAX, mxy = -FLT_MAX, mxz = -FLT_MAX;
    int ncand = 0;
    // the ring's points stay in registers: all loads are issued back to back, and the cell pass needs no second trip
    float4 pr[kVoxSlots];
    unsigned int cand_mask = 0;
    {
        // every slot's label and point are requested before the first label is looked at (index clamped into the ring: len >= 12 here);
        // with the candidate test next to its load the compiler waited for one label byte after the other -- 9 round trips instead of 1
        signed char lbs[kVoxSlots];
#pragma unroll
        for (int m = 0; m < kVoxSlots; m++) {
            const int i = tid + 256 * m, ic = i < len ? i : len - 1;
            lbs[m] = label[ic]; pr[m] = cl[ic];
        }
#pragma unroll
        for (int m = 0; m < kVoxSlots; m++) {
            const int i = tid + 256 * m;
            if (i >= len) pr[m] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i >= c_lo && i <= c_hi && i < len && lbs[m] <= 0) cand_mask |= 1u << m;
        }
    }
#pragma unroll
    for (int m = 0; m < kVoxSlots; m++) {
        if ((cand_mask >> m) & 1u) {
            const float4 p = pr[m];
            mnx = fminf(mnx, p.x); mny = fminf(mny, p.y); mnz = fminf(mnz, p.z);
            mxx = fmaxf(mxx, p.x); mxy = fmaxf(mxy, p.y); mxz = fmaxf(mxz, p.z);
            ncand++;
        }
    }
    VT(1)
    float *fs = (float *)scr;   // [4 waves][6] + counts
    mnx = wave_min_f(mnx); mny = wave_min_f(mny); mnz = wave_min_f(mnz);
    mxx = wave_max_f(mxx); mxy = wave_max_f(mxy); mxz = wave_max_f(mxz);
    ncand = wave_sum_i(ncand);
    if (lane == 0) {
        fs[wave * 6 + 0] = mnx; fs[wave * 6 + 1] = mny; fs[wave * 6 + 2] = mnz;
        fs[wave * 6 + 3] = mxx; fs[wave * 6 + 4] = mxy; fs[wave * 6 + 5] = mxz;
        scr[32 + wave] = ncand;
    }
    __syncthreads();
    ncand = scr[32] + scr[33] + scr[34] + scr[35];
    if (ncand == 0) {
        if (tid == 0) b.lf_n[s * 64 + r] = 0;
        return;
    }
    mnx = fminf(fminf(fs[0], fs[6]), fminf(fs[12], fs[18]));
    mny = fminf(fminf(fs[1], fs[7]), fminf(fs[13], fs[19]));
    mnz = fminf(fminf(fs[2], fs[8]), fminf(fs[14], fs[20]));
    mxx = fmaxf(fmaxf(fs[3], fs[9]), fmaxf(fs[15], fs[21]));
    mxy = fmaxf(fmaxf(fs[4], fs[10]), fmaxf(fs[16], fs[22]));
    mxz = fmaxf(fmaxf(fs[5], fs[11]), fmaxf(fs[17], fs[23]));
    const float inv_leaf = 5.0f;
    const int minb0 = (int)floorf(mnx * inv_leaf), minb1 = (int)floorf(mny * inv_leaf), minb2 = (int)floorf(mnz * inv_leaf);
    const int div0 = (int)floorf(mxx * inv_leaf) - minb0 + 1, div1 = (int)floorf(mxy * inv_leaf) - minb1 + 1;
    const int mul1 = div0, mul2 = div0 * div1;
    // bucket of a cell for the bucket sort: its index shifted so that at most kVoxBuckets buckets cover the bounding box
    const unsigned long long ncell = (unsigned long long)div0 * (unsigned long long)div1 * (unsigned long long)((int)floorf(mxz * inv_leaf) - minb2 + 1);
    const int cell_bits = ncell > 1ull ? 64 - __clzll((long long)(ncell - 1ull)) : 0;
    const int bshift = cell_bits > kVoxBucketBits ? cell_bits - kVoxBucketBits : 0;
    // ---- cells (registers), cell of the last lane of every (slot, wave) for the neighbour test across waves
    unsigned int cellr[kVoxSlots];
#pragma unroll
    for (int m = 0; m < kVoxSlots; m++) {
        unsigned int cell = ~0u;
        if ((cand_mask >> m) & 1u) {
            const float4 p = pr[m];
            const int i0 = (int)(floorf(p.x * inv_leaf) - (float)minb0);
            const int i1 = (int)(floorf(p.y * inv_leaf) - (float)minb1);
            const int i2 = (int)(floorf(p.z * inv_leaf) - (float)minb2);
            cell = (unsigned int)(i0 + i1 * mul1 + i2 * mul2);
        }
        cellr[m] = cell;
        if (lane == 63) lastc[m * 4 + wave] = cell;
    }
    // small instantiation: 8 bytes of LDS per segment (the kernel is bound by resident workgroups -- 3 per CU at 46 KB measured 6.2 ms,
    // 2 per CU 8.8 ms).  A scattered key is one word, (cell & (2^bshift - 1)) << 12 | first index: inside a bucket the cell bits above
    // bshift are equal, so this word orders a bucket's keys as (cell, first index) does, and the ranking compares words.  The sorted
    // array holds what the accumulation reads, the first index, and bit 15 = "first segment of its voxel" (found while ranking).
    unsigned long long *tmp = keys + kVoxBucketSegs;                                        // big only: scattered keys
    unsigned int *wsc = (unsigned int *)keys;                                               // small only: scattered key words
    unsigned short *bkt = (unsigned short *)((unsigned char *)keys + kVoxBucketSegs * 4);   //             and their buckets
    unsigned short *srt = (unsigned short *)((unsigned char *)keys + kVoxBucketSegs * 6);   // small only: sorted segments
    int *hist = kSmall ? (int *)((unsigned char *)keys + kVoxBucketSegs * 8) : (int *)(keys + 2 * kVoxBucketSegs);
    __syncthreads();            // fs / scr[32..35] are read, lastc is written
    VT(2)
    // ---- segment heads: a candidate whose predecessor in the ring is not a candidate of the same cell
    unsigned int head_mask = 0;
#pragma unroll
    for (int m = 0; m < kVoxSlots; m++) {
        const int i = tid + 256 * m;
        unsigned int prev = (unsigned int)__shfl_up((int)cellr[m], 1);
        if (lane == 0) prev = wave > 0 ? lastc[m * 4 + wave - 1] : (m > 0 ? lastc[(m - 1) * 4 + 3] : ~0u);
        const bool cand = cellr[m] != ~0u;
        const bool cont = cand && i > 0 && prev == cellr[m];
        const bool head = cand && !cont;
        const unsigned long long hm = __ballot(head), cm = __ballot(cont);
        if (lane == 0) { contw[m * 4 + wave] = cm; scr[64 + m * 4 + wave] = __popcll(hm); }
        if (head) head_mask |= 1u << m;
    }
    if (tid < 2) contw[kVoxSlots * 4 + tid] = 0ull;
    __syncthreads();
    // position of a head in ring order = heads of the earlier (slot, wave) pairs + heads below it in its own ballot
    // (lane l of every wave scans the count of pair l; the big instantiation alone needs the bases, for its bitonic network)
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int hc = lane < kVoxSlots * 4 ? scr[64 + lane] : 0;
    const int hincl = wave_scan_incl_dpp(hc);
    const int nseg = __builtin_amdgcn_readlane(hincl, 63);
    int hbase[kVoxSlots];
    if (!kSmall) {
#pragma unroll
        for (int m = 0; m < kVoxSlots; m++) hbase[m] = __builtin_amdgcn_readlane(hincl - hc, m * 4 + wave_u);
    }
    int np2 = next_pow2(nseg);
    if (np2 < 2) np2 = 2;
    // the small instantiation's key word holds bshift + 12 <= 32 bits: up to 2^31 cells
    const bool bucket_path = nseg <= kVoxBucketSegs && ncell <= (kSmall ? 0x80000000ull : 0xffffffffull);
    if (kSmall && !bucket_path) {
        if (tid == 0) b.vox_todo[1 + atomicAdd(&b.vox_todo[0], 1)] = (s << 6) | r;    // needs the bitonic network: big instantiation
        return;
    }
    if (bucket_path && kSmall) {
        // 2048 counters of 16 bits, two per word (a ring has at most 2304 segments, so neither a count nor a cursor carries into its
        // neighbour): thread tid owns the 8 counters of words 4 tid .. 4 tid + 3
        uint4 *hw4 = (uint4 *)hist;
        unsigned int *hw = (unsigned int *)hist;
        const unsigned short *h16 = (const unsigned short *)hist;
        hw4[tid] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < kVoxSlots; m++)
            if ((head_mask >> m) & 1u) { const unsigned int bk = cellr[m] >> bshift; atomicAdd(&hw[bk >> 1], 1u << ((bk & 1u) * 16u)); }
        __syncthreads();
        VT(3)
        const uint4 cw = hw4[tid];
        const unsigned int c0 = cw.x & 0xffffu, c1 = cw.x >> 16, c2 = cw.y & 0xffffu, c3 = cw.y >> 16;
        const unsigned int c4 = cw.z & 0xffffu, c5 = cw.z >> 16, c6 = cw.w & 0xffffu, c7 = cw.w >> 16;
        const int sum = (int)(c0 + c1 + c2 + c3 + c4 + c5 + c6 + c7);
        const int incl_b = wave_scan_incl_dpp(sum);
        if (lane == 63) scr[44 + wave] = incl_b;
        __syncthreads();
        unsigned int run = (unsigned int)(incl_b - sum);
        for (int w = 0; w < wave; w++) run += (unsigned int)scr[44 + w];
        uint4 ew;
        { const unsigned int e0 = run, e1 = e0 + c0, e2 = e1 + c1, e3 = e2 + c2, e4 = e3 + c3, e5 = e4 + c4, e6 = e5 + c5, e7 = e6 + c6;
          ew = make_uint4(e0 | (e1 << 16), e2 | (e3 << 16), e4 | (e5 << 16), e6 | (e7 << 16)); }
        hw4[tid] = ew;
        __syncthreads();
        const unsigned int cmask = (1u << bshift) - 1u;
#pragma unroll
        for (int m = 0; m < kVoxSlots; m++)
            if ((head_mask >> m) & 1u) {
                const unsigned int bk = cellr[m] >> bshift, sh = (bk & 1u) * 16u;
                const unsigned int q = (atomicAdd(&hw[bk >> 1], 1u << sh) >> sh) & 0xffffu;
                wsc[q] = ((cellr[m] & cmask) << 12) | (unsigned int)(tid + 256 * m);
                bkt[q] = (unsigned short)bk;
            }
        __syncthreads();
        // a cursor is now the end of its bucket = the start of the next one.  Every key counts the smaller keys of its bucket and takes that
        // place: the exact (cell, first index) order whatever the arrival order was.  A wave runs as long as its largest bucket (a bucket
        // spans a few rows of x, so a ring that runs along x puts dozens of segments into one); a trip is one LDS read and two compares,
        // the second of which counts the keys of smaller cells: a key that has only those below it starts a voxel.
        for (int t = tid; t < nseg; t += 256) {
            const unsigned int k = wsc[t], kc = k & ~0xfffu;
            const int bk = bkt[t];
            const int lo = bk > 0 ? h16[bk - 1] : 0, hi = h16[bk];
            int less = 0, lessc = 0;
            // (four keys a trip, read together and masked behind the bucket's end, measured slower: 3.05 against 2.99 ms)
            for (int u = lo; u < hi; u++) { const unsigned int ku = wsc[u]; less += ku < k ? 1 : 0; lessc += ku < kc ? 1 : 0; }
            srt[lo + less] = (unsigned short)((k & 0xfffu) | (less == lessc ? 0x8000u : 0u));
        }
        __syncthreads();
    } else if (!kSmall && bucket_path) {
        for (int i = tid; i < kVoxBuckets; i += 256) hist[i] = 0;
        __syncthreads();
#pragma unroll
        for (int m = 0; m < kVoxSlots; m++)
            if ((head_mask >> m) & 1u) atomicAdd(&hist[cellr[m] >> bshift], 1);
        __syncthreads();
        VT(3)
        constexpr int kPer = kVoxBuckets / 256;
        int c[kPer], sum = 0;
#pragma unroll
        for (int q = 0; q < kPer; q++) { c[q] = hist[tid * kPer + q]; sum += c[q]; }
        const int incl_b = wave_scan_incl_dpp(sum);
        if (lane == 63) scr[44 + wave] = incl_b;
        __syncthreads();
        int run = incl_b - sum;
        for (int w = 0; w < wave; w++) run += scr[44 + w];
#pragma unroll
        for (int q = 0; q < kPer; q++) { hist[tid * kPer + q] = run; run += c[q]; }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < kVoxSlots; m++)
            if ((head_mask >> m) & 1u) {
                const int q = atomicAdd(&hist[cellr[m] >> bshift], 1);
                tmp[q] = ((unsigned long long)cellr[m] << 32) | (unsigned int)(tid + 256 * m);
            }
        __syncthreads();
        // a cursor is now the end of its bucket = the start of the next one; ranking as above, on the whole 64-bit keys
        for (int t = tid; t < nseg; t += 256) {
            const unsigned long long k = tmp[t];
            const int bk = (int)((unsigned int)(k >> 32) >> bshift);
            const int lo = bk > 0 ? hist[bk - 1] : 0, hi = hist[bk];
            int less = 0;
            for (int u = lo; u < hi; u++) less += tmp[u] < k ? 1 : 0;
            keys[lo + less] = k;
        }
        __syncthreads();
    } else if (!kSmall) {
#pragma unroll
        for (int m = 0; m < kVoxSlots; m++) {
            const unsigned long long hm = __ballot((head_mask >> m) & 1u);
            if ((head_mask >> m) & 1u)
                keys[hbase[m] + __popcll(hm & ((1ull << lane) - 1ull))] = ((unsigned long long)cellr[m] << 32) | (unsigned int)(tid + 256 * m);
        }
        for (int k = nseg + tid; k < np2; k += 256) keys[k] = ~0ull;
        __syncthreads();
        VT(3)
        bitonic_sort_u64(keys, np2);
    }
    VT(4)
    // ---- runs of equal cell over the sorted segments -> output voxels; vstart[o] = first sorted segment of voxel o
    int *vstart = bucket_path && !kSmall ? (int *)(keys + kVoxBucketSegs) : nullptr;   // big: the scattered copy is dead now
    unsigned short *vstart16 = (unsigned short *)hist;                                 // small: the bucket counters are dead after the ranking
    constexpr int kRounds = (kVoxBucketSegs + 255) / 256;
    const int rounds = (nseg + 255) / 256;
    int n_out = 0;
    unsigned int st_mask = 0;          // bit j: sorted segment tid + 256 j starts a voxel (computed once, used by both passes)
    if (bucket_path) {
        // voxel starts per round and wave -> prefix in sorted order (round, wave, lane)
        for (int j = 0; j < rounds; j++) {
            const int t = tid + 256 * j;
            bool st;
            if (kSmall) st = t < nseg && (srt[t] & 0x8000u) != 0u;
            else st = t < nseg && (t == 0 || (unsigned int)(keys[t] >> 32) != (unsigned int)(keys[t - 1] >> 32));
            const unsigned long long sm = __ballot(st);
            if (lane == 0) scr[128 + j * 4 + wave] = __popcll(sm);
            if (st) st_mask |= 1u << j;
        }
    }
    __syncthreads();
    float4 *outp = b.lf_tmp + off + rbeg;
    // one segment's points, added one after the other in index order (four requested at a time)
    auto add_run = [&](int i0, float &sx, float &sy, float &sz, float &si, int &cnt) {
        const int rl = vox_run_length(contw, i0);
        for (int b4 = 0; b4 < rl; b4 += 4) {
            float4 q4[4];
#pragma unroll
            for (int k = 0; k < 4; k++) q4[k] = b4 + k < rl ? cl[i0 + b4 + k] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < 4; k++) if (b4 + k < rl) { sx += q4[k].x; sy += q4[k].y; sz += q4[k].z; si += q4[k].w; }
        }
        cnt += rl;
    };
    VT(5)
    if (bucket_path) {
        // (lane l of every wave scans the count of pair l, as for the heads)
        const int oc = lane < rounds * 4 ? scr[128 + lane] : 0;
        const int oincl = wave_scan_incl_dpp(oc);
        n_out = __builtin_amdgcn_readlane(oincl, 63);
#pragma unroll
        for (int j = 0; j < kRounds; j++) {
            if (j >= rounds) break;
            const int t = tid + 256 * j;
            const bool st = (st_mask >> j) & 1u;
            const int obase = __builtin_amdgcn_readlane(oincl - oc, j * 4 + wave_u);
            const unsigned long long sm = __ballot(st);
            if (st) { const int o = obase + __popcll(sm & ((1ull << lane) - 1ull)); if (kSmall) vstart16[o] = (unsigned short)t; else vstart[o] = t; }
        }
        __syncthreads();
        // one voxel per thread and round: its segments [vstart[v], vstart[v + 1]) in sorted order, every segment's points in index order
        for (int v = tid; v < n_out; v += 256) {
            int t0, t1;
            if (kSmall) { t0 = vstart16[v]; t1 = v + 1 < n_out ? (int)vstart16[v + 1] : nseg; }
            else { t0 = vstart[v]; t1 = v + 1 < n_out ? vstart[v + 1] : nseg; }
            float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
            int cnt = 0;
            for (int u = t0; u < t1; u++) {
                const int i0 = kSmall ? (int)(srt[u] & 0xfffu) : (int)(keys[u] & 0xffffffffull);
                add_run(i0, sx, sy, sz, si, cnt);
            }
            const float fc = (float)cnt;
            outp[v] = make_float4(sx / fc, sy / fc, sz / fc, si / fc);
        }
    } else if (!kSmall) {
        // long rings: contiguous ranges of sorted segments per thread (serial prefix of the voxel starts)
        const int chunk2 = (np2 + 255) / 256;
        const int t_lo = tid * chunk2, t_hi = min(t_lo + chunk2, nseg);
        int nstart = 0;
        for (int t = t_lo; t < t_hi; t++) {
            const unsigned int c = (unsigned int)(keys[t] >> 32);
            if (t == 0 || c != (unsigned int)(keys[t - 1] >> 32)) nstart++;
        }
        const int incl = wave_scan_incl(nstart);
        __syncthreads();
        if (lane == 63) scr[48 + wave] = incl;
        __syncthreads();
        int base = incl - nstart;
        for (int w = 0; w < wave; w++) base += scr[48 + w];
        n_out = scr[48] + scr[49] + scr[50] + scr[51];
        int o = base;
        for (int t = t_lo; t < t_hi; t++) {
            const unsigned int c = (unsigned int)(keys[t] >> 32);
            if (t == 0 || c != (unsigned int)(keys[t - 1] >> 32)) {
                float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
                int cnt = 0;
                for (int u = t; u < nseg && (unsigned int)(keys[u] >> 32) == c; u++) {
                    add_run((int)(keys[u] & 0xffffffffull), sx, sy, sz, si, cnt);
                }
                const float fc = (float)cnt;
                outp[o++] = make_float4(sx / fc, sy / fc, sz / fc, si / fc);
            }
        }
    }
    VT(6)
#ifdef LMONO_VOX_PROF
    if (blockIdx.x == 20 && blockIdx.y == 3 && tid == 0) printf("VOX len %d nseg %d nout %d | load %lld bbox+cell %lld heads %lld sort %lld runs %lld accum %lld\n", len, nseg, n_out, vt[1]-vt[0], vt[2]-vt[1], vt[3]-vt[2], vt[4]-vt[3], vt[5]-vt[4], vt[6]-vt[5]);
#endif
    if (tid == 0) b.lf_n[s * 64 + r] = n_out;
}

// ------------------------------------------------------------------------------------------------
// Line tables of a feature cloud (line = int(intensity), what laserOdometry reads as the scan line):
//   first_ge[t] = first index whose line is >= t, last_le[t] = last index whose line is <= t  (t = 0..65).
// The odometry walk around a nearest point of line ra visits exactly the index window (last_le[ra-3], first_ge[ra+3])
// provided no point precedes a point whose line is >= 3 lower ("regular"); irregular clouds are flagged and walked
// in array order instead.  Lines are not monotone in general: A-LOAM's relTime can be negative (line = ring - 1).
// ------------------------------------------------------------------------------------------------

// compact_scan's feed: what happens to the two "last" clouds (cld 0: less sharp, 1: less flat) while their points pass through its copy loops.  The
// points are counted per (line, azimuth bin) and feed the elevation bounds while the loop holds them, instead of the cloud being read once more; tables
// and scatter follow the loop.  The feed's state (the 16-bit counters of line_index.hip) serves one cloud after the other.
//   reset(cld, n)   before the cloud's copy loop, by every thread; a barrier of compact_scan follows before the first point()
//   point(ok, p)    every point the loop writes, called by WHOLE waves (ok = false: a lane without a point)
//   finish(cld, n)  behind the loop, by every thread; holds barriers
struct CompactIndexFeed {
    const BatchView &b;
    LiLds L;
    int s;
    bool on;                       // false: a cloud of more than 65535 points, copied plainly and listed for the full-width launch
    __device__ __forceinline__ void reset(int cld, int n)
    {
        on = n <= 65535;
        if (on) li_reset<true>(L);
        else if (threadIdx.x == 0) b.li_todo[1 + atomicAdd(&b.li_todo[0], 1)] = s * 2 + cld;
    }
    __device__ __forceinline__ void point(bool ok, const float4 &p) { if (on) li_count<true>(L, ok, p.x, p.y, p.z, p.w); }
    __device__ __forceinline__ void finish(int cld, int n)
    {
        if (!on) return;
        __syncthreads();
        li_tables<true>(b, L, s, cld != 0, n);
        // this workgroup's own stores (the cloud) are read back by the scatter: they are out of the vector unit before anybody loads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        li_scatter<true>(b, L, s, cld != 0, n);
    }
};

// one scan's feature clouds compacted and indexed by the kLiT threads of k_compact_index
__device__ __forceinline__ void compact_scan(const BatchView &b, int s, CompactIndexFeed &feed)
{
    constexpr int kT = kLiT;
    const int tid = threadIdx.x;
    const int64_t off = b.off[s];
    constexpr int NE = kMaxRings * kSectors;   // 384
    __shared__ int pre_sh[NE + 1], pre_ls[NE + 1], pre_fl[NE + 1], pre_lf[kMaxRings + 1];
    const int *nsh = b.sel_sharp_n + s * NE;
    const int *nfl = b.sel_flat_n + s * NE;
    // four exclusive prefixes, one per wave: (ring, sector) counts of sharp (<= 2), less sharp, flat; ring counts of less flat
    {
        const int lane = tid & 63, wave = tid >> 6;
        constexpr int kPer = NE / 64;   // 6 consecutive entries per lane
        int c[kPer], sum = 0;
        if (wave < 4) {
        // one source array per wave, six unconditional loads per lane in flight together
        const int *srcp = wave <= 1 ? nsh : (wave == 2 ? nfl : b.lf_n + s * 64);
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            const int e = lane * kPer + q;
            const bool on = wave < 3 || e < kMaxRings;
            c[q] = srcp[on ? e : 0];
            if (!on) c[q] = 0;
        }
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            if (wave == 0) c[q] = min(c[q], 2);
            sum += c[q];
        }
        const int incl = wave_scan_incl(sum);
        int run = incl - sum;
        int *dst = wave == 0 ? pre_sh : (wave == 1 ? pre_ls : (wave == 2 ? pre_fl : pre_lf));
        const int n_e = wave == 3 ? kMaxRings : NE;
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            const int e = lane * kPer + q;
            if (e < n_e) dst[e] = run;
            run += c[q];
        }
        if (lane == 63) dst[n_e] = run;
        }
    }
    __syncthreads();
    const float4 *cl = b.cloud + off;
    float4 *sharp = b.sharp + (size_t)s * kMaxSharp;
    float4 *ls = b.less_sharp + (size_t)s * kMaxLessSharp;
    float4 *flat = b.flat + (size_t)s * kMaxFlat;
    float4 *lf = b.less_flat + off;
    const int *ssel = b.sel_sharp + (size_t)s * NE * 20;
    const int *fsel = b.sel_flat + (size_t)s * NE * 4;
    // line tables of the two "last" clouds are gathered while the points pass through (first / last index of every line)
    __shared__ int s_first[2][66], s_last[2][66], s_flag[2], s_rb[kMaxRings + 1];
    if (tid < 66) { s_first[0][tid] = INT_MAX; s_last[0][tid] = -1; s_first[1][tid] = INT_MAX; s_last[1][tid] = -1; }
    if (tid < 2) s_flag[tid] = 0;
    if (tid >= 128 && tid < 128 + kMaxRings + 1) s_rb[tid - 128] = b.ring_begin[s * 65 + tid - 128];
    const int n_ls = pre_ls[NE], n_lf = pre_lf[kMaxRings];
    feed.reset(0, n_ls);
    __syncthreads();
    // four selection slots per thread and turn: the counts come from the LDS prefixes, the index loads and then the point gathers are issued
    // together (behind per-slot guards the compiler waits for every load in turn: three dependent round trips per slot, 30 slots per thread)
    // (NE * 20 is a multiple of 64: the lanes of a wave make the same trips)
    static_assert(NE * 20 % 64 == 0, "feed.point() needs whole waves");
    for (int x0 = tid; x0 < NE * 20; x0 += 4 * kT) {
        int pos[4], idx[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int x = x0 + kT * q, e = x / 20, k = x % 20;
            pos[q] = (x < NE * 20 && k < pre_ls[e + 1] - pre_ls[e]) ? pre_ls[e] + k : -1;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) idx[q] = ssel[pos[q] >= 0 ? x0 + kT * q : 0];
        float4 p4[4];
#pragma unroll
        for (int q = 0; q < 4; q++) { const float4 *src = pos[q] >= 0 ? cl + idx[q] : b.cloud; p4[q] = *src; }      // (an unused slot reads the batch's first point)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float4 p = p4[q];
            if (pos[q] >= 0) {
                const int x = x0 + kT * q, e = x / 20, k = x % 20;
                ls[pos[q]] = p;
                if (k < 2) sharp[pre_sh[e] + k] = p;
                int v = (int)p.w;
                v = v < 0 ? 0 : (v > 65 ? 65 : v);
                atomicMin(&s_first[0][v], pos[q]);
                atomicMax(&s_last[0][v], pos[q]);
            }
            feed.point(pos[q] >= 0, p);
        }
    }
    for (int x0 = tid; x0 < NE * 4; x0 += 2 * kT) {
        int pos[2], idx[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int x = x0 + kT * q, e = x / 4, k = x % 4;
            pos[q] = (x < NE * 4 && k < pre_fl[e + 1] - pre_fl[e]) ? pre_fl[e] + k : -1;
        }
#pragma unroll
        for (int q = 0; q < 2; q++) idx[q] = fsel[pos[q] >= 0 ? x0 + kT * q : 0];
        float4 p2[2];
#pragma unroll
        for (int q = 0; q < 2; q++) { const float4 *src = pos[q] >= 0 ? cl + idx[q] : b.cloud; p2[q] = *src; }
#pragma unroll
        for (int q = 0; q < 2; q++) if (pos[q] >= 0) flat[pos[q]] = p2[q];
    }
    // the feed's state serves one cloud after the other
    feed.finish(0, n_ls);
    __syncthreads();
    feed.reset(1, n_lf);
    __syncthreads();
    // less-flat cloud = the rings' voxel outputs back to back: every thread finds the ring of its output index by a binary
    // search over the ring prefix (all loads independent, four per thread in flight)
    for (int base = 0; base < n_lf; base += 4 * kT) {      // uniform trip count: feed.point() needs whole waves
        const int j0 = base + tid;
        float4 v4[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int j = j0 + kT * q;
            v4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < n_lf) {
                int lo = 0, hi = kMaxRings;
                while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (pre_lf[mid] <= j) lo = mid; else hi = mid; }
                v4[q] = b.lf_tmp[off + s_rb[lo] + (j - pre_lf[lo])];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int j = j0 + kT * q;
            if (j < n_lf) {
                lf[j] = v4[q];
                int v = (int)v4[q].w;
                v = v < 0 ? 0 : (v > 65 ? 65 : v);
                atomicMin(&s_first[1][v], j);
                atomicMax(&s_last[1][v], j);
            }
            feed.point(j < n_lf, v4[q]);
        }
    }
    feed.finish(1, n_lf);
    if (tid == 0) {
        b.feat_n[s * 4 + 0] = pre_sh[NE]; b.feat_n[s * 4 + 1] = n_ls;
        b.feat_n[s * 4 + 2] = pre_fl[NE]; b.feat_n[s * 4 + 3] = n_lf;
    }
    __syncthreads();
    // irregular iff some line a >= b + 3 starts before line b ends (see above)
    for (int x = tid; x < 2 * 66 * 66; x += kT) {
        const int cld = x / (66 * 66), y = x % (66 * 66), a = y / 66, bb = y % 66;
        if (a >= bb + 3 && s_first[cld][a] < s_last[cld][bb]) s_flag[cld] = 1;
    }
    __syncthreads();
    if (tid == 0 || tid == 64) {
        const int cld = tid >> 6;
        const int n = cld ? n_lf : n_ls;
        int *first_ge = b.line_first_ge + (size_t)(s * 2 + cld) * 66, *last_le = b.line_last_le + (size_t)(s * 2 + cld) * 66;
        int m = n;
        for (int t = 65; t >= 0; t--) { m = min(m, s_first[cld][t] == INT_MAX ? n : s_first[cld][t]); first_ge[t] = m; }
        int M = -1;
        for (int t = 0; t <= 65; t++) { M = max(M, s_last[cld][t]); last_le[t] = M; }
        if (s_flag[cld]) atomicOr(b.status + s, kStatusIrregularLines);
    }
}

// Compaction and the 16-bit line index as ONE kernel (round 5, VERDICT r4 #2a): a workgroup compacts its scan's feature clouds and indexes the two "last"
// clouds right away.  Round 5 measured the fusion as neutral against the two stand-alone kernels (1.90 + 2.02 -> 3.92 ms per pass; that pair was removed
// in round 9) and put that down to traffic; round 8 found the cause in
// the kernel's resources: 91 VGPRs, so ONE 1024-thread workgroup per CU (the stand-alone kernels ran two), and the re-reads of the clouds it had just
// written were not served by L2 (1.25 MB fetched per scan for 0.55 MB of clouds).  Since round 8 (profiles/r8/NOTES.md):
//   * the copy loops of compact_scan count the points per (line, bin) and feed the elevation bounds while they hold them (CompactIndexFeed): the
//     separate count pass over the written cloud is gone, 0.94 MB fetched per scan;
//   * the phases are separate functions over LDS state with nothing carried between them in registers: 52 VGPRs, 48 B of scratch, 57.5 KB of LDS,
//     TWO workgroups per CU (the launch bound pins 8 waves per SIMD; the occupancy query of -DLMONO_TILE_PROF builds reports it);
//   * the start table leaves LDS in rows (li_tables).
// 3.97 -> 3.10 ms per pass: 10.9 GB moved in about 3.1 ms, 3.5 TB/s, where one workgroup per CU moved 12.7 GB in 3.97 ms.  Residency and its own chain
// of phases bound it first, bytes second.  The 16-bit counters serve one cloud after the other; a cloud of more than 65535 points is copied plainly and
// goes to the full-width launch's list (k_line_index<false>, line_index.hip).
__global__ __launch_bounds__(kLiT, 8) void k_compact_index(BatchView b)
{
    extern __shared__ __align__(16) int s_cnt[];
    __shared__ int s_wsum[kLiT / 64], s_emin[66], s_emax[66];
    CompactIndexFeed feed = { b, { s_cnt, s_wsum, s_emin, s_emax }, b.scan0 + (int)blockIdx.x, false };
    compact_scan(b, feed.s, feed);
}

} // namespace lmono
