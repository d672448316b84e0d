// track.hip -- image feature tracker kernels (gfx950, wave64): FeatureTracker::trackImage of the mono path
// (mono_lidar_mapping/src/image_process/FeatureTracker.cc:189-433, use_rejectF = 0).  DESIGN.md 6e holds the written
// definition these kernels and tests/track_ref.py implement: every accumulation is an exact integer, every remaining
// floating-point step one IEEE fp32 / fp64 operation in a fixed order (the library is built with -ffp-contract=off).
//   k_trk_grey      cv::cvtColor BGR2GRAY (:193) or a copy of an 8-bit grey frame into level 0 of the current pyramid
//   k_trk_pyrdown   cv::pyrDown: separable [1 4 6 4 1], BORDER_REFLECT_101, (sum + 128) >> 8
//   k_trk_scharr    [3 10 3] (x) [-1 0 1] derivatives of a level as int16; a level and its two derivative planes are
//                   written once per frame and become the previous pyramid of the next frame by pointer swap
//   k_trk_lk        cv::calcOpticalFlowPyrLK (:218, :223), one wave per (stream, point): the 441 patch pixels live 7 per
//                   lane in registers for all iterations, integer products, integer wave sums, the 2 x 2 solve in fp64 in
//                   every lane; levels and iterations loop inside the kernel
//   k_trk_reject    rejectWithF (:259-262, :435-503; track_reject.hip), only when a stream of the batch has it switched on
//   k_trk_update    forward-backward / inBorder test (:226-243), compaction (:245-248), track_cnt++ (:251), setMask
//                   (:55-84, stable order), one workgroup per stream
//   k_trk_response  cv::cornerMinEigenVal (block 3, Sobel 3) on an LDS tile with halo + the maximum over unmasked pixels
//   k_trk_nms       threshold, 3 x 3 local maximum, mask test -> (value, pixel) keys
//   k_trk_select    cv::goodFeaturesToTrack's greedy pass: strongest live key, all lanes suppress what lies within MIN_DIST
//   k_trk_finish    new ids (:291-297), liftProjective (:172-187), ptsVelocity (:94-133), the packed record array
#pragma once
#include "common.hpp"
#include "colour.hip"

namespace lmono {

constexpr int kTrkWin = 21, kTrkHalf = 10;
constexpr int kTrkLevels = 4;              // maxLevel 3
constexpr int kTrkIters = 30;
constexpr int kTrkMaxPts = LMONO_TRACK_MAX_POINTS;
constexpr int kTrkMaxRadius = 128;
constexpr int kTrkT = 256;
constexpr int kTrkTW = 64, kTrkTH = 16;    // response tile

struct TrkLevel { int w, h; unsigned char *img; short *dx, *dy; };
struct TrkPyr { TrkLevel lv[kTrkLevels]; };

struct TrkState {            // device-resident counters of one stream
    int n;                   // points carried from the previous frame
    int n_id;                // next feature id
    int n_kept;              // points that survived setMask this frame
    int quota;               // MAX_CNT - n_kept
    unsigned int max_bits;   // bit pattern of the largest positive unmasked response
    int n_cand, n_new, pad;
};

struct TrkJob {
    int w, h, n_levels, max_cnt, min_dist, format;
    int lk_n;                          // >= 0: diagnostic LK call on lk_pts; < 0: the stream's own points
    double dt;
    ColourCam cam;
    TrkPyr prev, cur;
    const unsigned char *src;
    TrkState *st;
    float2 *pts, *un;                  // points of the previous frame / their undistorted positions
    int *ids, *cnt;
    const float2 *lk_pts;
    float2 *cur_pts, *rev_pts;
    unsigned char *st_f, *st_b;
    int2 *kept_pix;
    float *resp;
    unsigned long long *cand;
    int2 *new_pts;
    lmono_track_record *rec;
    int *n_out;
    int hw[kTrkMaxRadius + 1];         // cv::circle(.., MIN_DIST, .., -1): half width of row |dy|
    // rejectWithF (track_reject.hip); rej_st == nullptr: off
    unsigned char *rej_st;             // one status byte per point slot
    int *rej_stats;                    // valid hypotheses, best hypothesis, gate-1 inliers, kept after gate 2
    double *rej_F;                     // [9] row-major
    double rej_thr2, rej_dis, rej_focal;
    int rej_nhyp, rej_n;               // rej_n >= 0: diagnostic call on rej_n given pairs
    unsigned int rej_seed, rej_key;    // rej_key: frames tracked since the last reset
    const float2 *rej_prev, *rej_cur;
};

__device__ __forceinline__ int trk_reflect(int i, int n)
{
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// cv::cvtColor BGR2GRAY on 8-bit data (shared with keyframe.hip)
__device__ __forceinline__ int trk_bgr_to_grey(int b, int g, int r) { return (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14; }

__global__ __launch_bounds__(kTrkT) void k_trk_grey(const TrkJob *jobs)
{
    const TrkJob &j = jobs[blockIdx.y];
    const int np = j.w * j.h;
    unsigned char *dst = j.cur.lv[0].img;
    for (int i = blockIdx.x * kTrkT + threadIdx.x; i < np; i += gridDim.x * kTrkT) {
        if (j.format == 0) dst[i] = j.src[i];
        else {
            const int b = j.src[3 * (size_t)i], g = j.src[3 * (size_t)i + 1], r = j.src[3 * (size_t)i + 2];
            dst[i] = (unsigned char)trk_bgr_to_grey(b, g, r);
        }
    }
}

__global__ __launch_bounds__(kTrkT) void k_trk_pyrdown(const TrkJob *jobs, int level)
{
    const TrkJob &j = jobs[blockIdx.y];
    if (level >= j.n_levels) return;
    const TrkLevel &S = j.cur.lv[level - 1], &D = j.cur.lv[level];
    const int np = D.w * D.h;
    for (int i = blockIdx.x * kTrkT + threadIdx.x; i < np; i += gridDim.x * kTrkT) {
        const int y = i / D.w, x = i - y * D.w;
        int xs[5];
#pragma unroll
        for (int k = 0; k < 5; k++) xs[k] = trk_reflect(2 * x + k - 2, S.w);
        int sum = 0;
#pragma unroll
        for (int r = 0; r < 5; r++) {
            const unsigned char *row = S.img + (size_t)trk_reflect(2 * y + r - 2, S.h) * S.w;
            const int h = row[xs[0]] + 4 * row[xs[1]] + 6 * row[xs[2]] + 4 * row[xs[3]] + row[xs[4]];
            sum += (r == 0 || r == 4) ? h : (r == 2 ? 6 * h : 4 * h);
        }
        D.img[i] = (unsigned char)((sum + 128) >> 8);
    }
}

__global__ __launch_bounds__(kTrkT) void k_trk_scharr(const TrkJob *jobs, int level)
{
    const TrkJob &j = jobs[blockIdx.y];
    if (level >= j.n_levels) return;
    const TrkLevel &L = j.cur.lv[level];
    const int np = L.w * L.h;
    for (int i = blockIdx.x * kTrkT + threadIdx.x; i < np; i += gridDim.x * kTrkT) {
        const int y = i / L.w, x = i - y * L.w;
        const int xm = trk_reflect(x - 1, L.w), xp = trk_reflect(x + 1, L.w);
        const unsigned char *r0 = L.img + (size_t)trk_reflect(y - 1, L.h) * L.w, *r1 = L.img + (size_t)y * L.w, *r2 = L.img + (size_t)trk_reflect(y + 1, L.h) * L.w;
        const int dx = 3 * (r0[xp] - r0[xm]) + 10 * (r1[xp] - r1[xm]) + 3 * (r2[xp] - r2[xm]);
        const int dy = 3 * (r2[xm] - r0[xm]) + 10 * (r2[x] - r0[x]) + 3 * (r2[xp] - r0[xp]);
        L.dx[i] = (short)dx;
        L.dy[i] = (short)dy;
    }
}

__device__ __forceinline__ long long wave_sum_ll(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct TrkWeights { int w00, w01, w10, w11; };
__device__ __forceinline__ TrkWeights trk_weights(float a, float b)
{
    TrkWeights t;
    t.w00 = __float2int_rn((1.f - a) * (1.f - b) * 16384.f);
    t.w01 = __float2int_rn(a * (1.f - b) * 16384.f);
    t.w10 = __float2int_rn((1.f - a) * b * 16384.f);
    t.w11 = 16384 - t.w00 - t.w01 - t.w10;
    return t;
}
// bilinear sample of the u8 level at window pixel (ox + wx, oy + wy), descaled by 9 bits; outside the level: REFLECT_101
__device__ __forceinline__ int trk_sample_img(const TrkLevel &L, int x, int y, const TrkWeights &t)
{
    const int x0 = trk_reflect(x, L.w), x1 = trk_reflect(x + 1, L.w);
    const unsigned char *r0 = L.img + (size_t)trk_reflect(y, L.h) * L.w, *r1 = L.img + (size_t)trk_reflect(y + 1, L.h) * L.w;
    return (r0[x0] * t.w00 + r0[x1] * t.w01 + r1[x0] * t.w10 + r1[x1] * t.w11 + 256) >> 9;
}
// the same of a derivative plane, descaled by 14 bits; outside the level: 0
__device__ __forceinline__ int trk_sample_der(const short *d, int w, int h, int x, int y, const TrkWeights &t)
{
    const bool xa = x >= 0 && x < w, xb = x + 1 >= 0 && x + 1 < w, ya = y >= 0 && y < h, yb = y + 1 >= 0 && y + 1 < h;
    const int v00 = (xa && ya) ? d[(size_t)y * w + x] : 0, v01 = (xb && ya) ? d[(size_t)y * w + x + 1] : 0;
    const int v10 = (xa && yb) ? d[(size_t)(y + 1) * w + x] : 0, v11 = (xb && yb) ? d[(size_t)(y + 1) * w + x + 1] : 0;
    return (v00 * t.w00 + v01 * t.w01 + v10 * t.w10 + v11 * t.w11 + 8192) >> 14;
}

// dir 0: previous -> current pyramid from pts (maxLevel 3); dir 1: current -> previous from cur_pts, started at pts (maxLevel 1)
__global__ __launch_bounds__(kTrkT) void k_trk_lk(const TrkJob *jobs, int dir)
{
    const TrkJob &j = jobs[blockIdx.y];
    const int pi = blockIdx.x * (kTrkT / kWave) + (threadIdx.x >> 6), lane = lane_id();
    const int n = j.lk_n >= 0 ? j.lk_n : j.st->n;
    if (pi >= n) return;
    const float2 *base = j.lk_n >= 0 ? j.lk_pts : j.pts;
    const TrkPyr &PI = dir == 0 ? j.prev : j.cur, &PJ = dir == 0 ? j.cur : j.prev;
    const float2 p0 = dir == 0 ? base[pi] : j.cur_pts[pi];
    float2 *out = dir == 0 ? j.cur_pts : j.rev_pts;
    unsigned char *st_out = dir == 0 ? j.st_f : j.st_b;
    if (dir == 1 && !j.st_f[pi]) {      // a point that failed forward is dropped whatever the backward pass says
        if (lane == 0) { out[pi] = base[pi]; st_out[pi] = 0; }
        return;
    }
    const int top = min(dir == 0 ? kTrkLevels - 1 : 1, j.n_levels - 1);
    int wx[7], wy[7];
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const int p = lane + 64 * k;
        wy[k] = p < 441 ? p / kTrkWin : -1;
        wx[k] = p < 441 ? p - (p / kTrkWin) * kTrkWin : 0;
    }
    float nx = 0.f, ny = 0.f;
    int status = 1;
    for (int level = top; level >= 0; level--) {
        const TrkLevel &LI = PI.lv[level], &LJ = PJ.lv[level];
        const float s = 1.f / (float)(1 << level);
        if (level == top) {
            const float2 q = dir == 0 ? p0 : base[pi];
            nx = q.x * s; ny = q.y * s;
        } else { nx = nx * 2.f; ny = ny * 2.f; }
        const float ppx = p0.x * s - (float)kTrkHalf, ppy = p0.y * s - (float)kTrkHalf;
        const float fx = floorf(ppx), fy = floorf(ppy);
        if (!(fx >= -(float)kTrkWin && fx < (float)LI.w && fy >= -(float)kTrkWin && fy < (float)LI.h)) { if (level == 0) status = 0; continue; }
        const int ox = (int)fx, oy = (int)fy;
        TrkWeights t = trk_weights(ppx - fx, ppy - fy);
        int I[7], Ix[7], Iy[7];
        int a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const bool v = wy[k] >= 0;
            const int x = ox + wx[k], y = oy + (v ? wy[k] : 0);
            I[k] = trk_sample_img(LI, x, y, t);
            Ix[k] = v ? trk_sample_der(LI.dx, LI.w, LI.h, x, y, t) : 0;
            Iy[k] = v ? trk_sample_der(LI.dy, LI.w, LI.h, x, y, t) : 0;
            a11 += Ix[k] * Ix[k]; a12 += Ix[k] * Iy[k]; a22 += Iy[k] * Iy[k];
        }
        const double sc = 1.0 / 1048576.0;
        const double A11 = (double)wave_sum_ll(a11) * sc, A12 = (double)wave_sum_ll(a12) * sc, A22 = (double)wave_sum_ll(a22) * sc;
        const double D = A11 * A22 - A12 * A12;
        const double tt = A11 - A22;
        const double min_eig = ((A22 + A11) - sqrt(tt * tt + 4.0 * (A12 * A12))) / (2.0 * kTrkWin * kTrkWin);
        if (min_eig < 1e-4 || D < (double)FLT_EPSILON) { if (level == 0) status = 0; continue; }
        float qx = nx - (float)kTrkHalf, qy = ny - (float)kTrkHalf;
        float pdx = 0.f, pdy = 0.f;
        for (int it = 0; it < kTrkIters; it++) {
            const float gx = floorf(qx), gy = floorf(qy);
            if (!(gx >= -(float)kTrkWin && gx < (float)LJ.w && gy >= -(float)kTrkWin && gy < (float)LJ.h)) { if (level == 0) status = 0; break; }
            const int jx = (int)gx, jy = (int)gy;
            t = trk_weights(qx - gx, qy - gy);
            int b1 = 0, b2 = 0;
#pragma unroll
            for (int k = 0; k < 7; k++) {
                const int x = jx + wx[k], y = jy + (wy[k] >= 0 ? wy[k] : 0);
                const int diff = trk_sample_img(LJ, x, y, t) - I[k];
                b1 += diff * Ix[k]; b2 += diff * Iy[k];
            }
            const double B1 = (double)wave_sum_ll(b1) * sc, B2 = (double)wave_sum_ll(b2) * sc;
            const float dx = (float)((A12 * B2 - A22 * B1) / D), dy = (float)((A12 * B1 - A11 * B2) / D);
            qx = qx + dx; qy = qy + dy;
            nx = qx + (float)kTrkHalf; ny = qy + (float)kTrkHalf;
            if ((double)dx * (double)dx + (double)dy * (double)dy <= 1e-4) break;
            if (it > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {
                nx = nx - dx * 0.5f; ny = ny - dy * 0.5f;
                break;
            }
            pdx = dx; pdy = dy;
        }
    }
    if (lane == 0) { out[pi] = make_float2(nx, ny); st_out[pi] = (unsigned char)status; }
}

__device__ __forceinline__ bool trk_in_circle(const int *hw, int r, int dx, int dy)
{
    dx = dx < 0 ? -dx : dx; dy = dy < 0 ? -dy : dy;
    return dy <= r && dx <= hw[dy];
}

// status of the forward-backward test and inBorder (:226-243) of point slot i
__device__ __forceinline__ int trk_keep(const TrkJob &j, int i)
{
    const float2 c = j.cur_pts[i], p = j.pts[i], q = j.rev_pts[i];
    const double dx = (double)(p.x - q.x), dy = (double)(p.y - q.y);
    const float rx = rintf(c.x), ry = rintf(c.y);
    return j.st_f[i] && j.st_b[i] && sqrt(dx * dx + dy * dy) <= 0.5 && 1.f <= rx && rx < (float)(j.w - 1) && 1.f <= ry && ry < (float)(j.h - 1);
}

// one workgroup of kTrkMaxPts threads per stream, thread i owns point slot i
__global__ __launch_bounds__(kTrkMaxPts) void k_trk_update(const TrkJob *jobs)
{
    __shared__ int s_flag[kTrkMaxPts], s_cnt[kTrkMaxPts], s_id[kTrkMaxPts], s_cnt2[kTrkMaxPts], s_id2[kTrkMaxPts], s_hw[kTrkMaxRadius + 1];
    __shared__ float2 s_pt[kTrkMaxPts], s_un[kTrkMaxPts], s_pt2[kTrkMaxPts], s_un2[kTrkMaxPts];
    __shared__ int2 s_px[kTrkMaxPts];
    const TrkJob &j = jobs[blockIdx.x];
    const int i = threadIdx.x, n = j.st->n, r = j.min_dist;
    for (int k = i; k <= r; k += kTrkMaxPts) s_hw[k] = j.hw[k];
    int keep = 0;
    float2 c = make_float2(0.f, 0.f), un = c;
    int id = 0, cnt = 0;
    if (i < n) {
        c = j.cur_pts[i];
        keep = trk_keep(j, i);
        if (j.rej_st) keep = keep && j.rej_st[i];
        id = j.ids[i]; cnt = j.cnt[i] + 1; un = j.un[i];
    }
    s_flag[i] = keep;
    __syncthreads();
    int rank = 0, m = 0;
    for (int k = 0; k < n; k++) { const int f = s_flag[k]; m += f; rank += (k < i) ? f : 0; }
    if (keep) { s_pt[rank] = c; s_un[rank] = un; s_id[rank] = id; s_cnt[rank] = cnt; }
    __syncthreads();
    // setMask: order by track count, descending, stable in the current index
    if (i < m) {
        const int ci = s_cnt[i];
        int pos = 0;
        for (int k = 0; k < m; k++) { const int ck = s_cnt[k]; pos += (ck > ci || (ck == ci && k < i)) ? 1 : 0; }
        const float2 p = s_pt[i];
        s_pt2[pos] = p; s_un2[pos] = s_un[i]; s_id2[pos] = s_id[i]; s_cnt2[pos] = ci;
        s_px[pos] = make_int2((int)rintf(p.x), (int)rintf(p.y));
    }
    s_flag[i] = i < m ? 1 : 0;        // alive
    __syncthreads();
    const int2 me = i < m ? s_px[i] : make_int2(0, 0);
    for (int k = 0; k < m; k++) {
        __syncthreads();
        if (s_flag[k] && i > k && i < m) {
            const int2 ck = s_px[k];
            if (trk_in_circle(s_hw, r, me.x - ck.x, me.y - ck.y)) s_flag[i] = 0;
        }
    }
    __syncthreads();
    rank = 0; int kept = 0;
    for (int k = 0; k < m; k++) { const int f = s_flag[k]; kept += f; rank += (k < i) ? f : 0; }
    if (i < m && s_flag[i]) {
        j.pts[rank] = s_pt2[i]; j.un[rank] = s_un2[i]; j.ids[rank] = s_id2[i]; j.cnt[rank] = s_cnt2[i];
        j.kept_pix[rank] = me;
    }
    if (i == 0) {
        TrkState *st = j.st;
        st->n_kept = kept; st->quota = j.max_cnt - kept; st->max_bits = 0u; st->n_cand = 0; st->n_new = 0;
    }
}

__global__ __launch_bounds__(kTrkT) void k_trk_response(const TrkJob *jobs)
{
    __shared__ unsigned char s_img[kTrkTH + 4][kTrkTW + 4];
    __shared__ short s_dx[kTrkTH + 2][kTrkTW + 2], s_dy[kTrkTH + 2][kTrkTW + 2];
    __shared__ int2 s_list[kTrkMaxPts];
    __shared__ int s_nlist, s_hw[kTrkMaxRadius + 1];
    const TrkJob &j = jobs[blockIdx.y];
    if (j.st->quota <= 0) return;
    const int w = j.w, h = j.h, tiles_x = (w + kTrkTW - 1) / kTrkTW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * kTrkTW, y0 = ty * kTrkTH;
    if (y0 >= h) return;
    const unsigned char *img = j.cur.lv[0].img;
    const int r = j.min_dist, n_kept = j.st->n_kept;
    if (threadIdx.x == 0) s_nlist = 0;
    for (int k = threadIdx.x; k <= r; k += kTrkT) s_hw[k] = j.hw[k];
    for (int k = threadIdx.x; k < (kTrkTH + 4) * (kTrkTW + 4); k += kTrkT) {
        const int ly = k / (kTrkTW + 4), lx = k - ly * (kTrkTW + 4);
        const int gy = y0 - 2 + ly, gx = x0 - 2 + lx;
        s_img[ly][lx] = (gy >= 0 && gy < h && gx >= 0 && gx < w) ? img[(size_t)gy * w + gx] : (unsigned char)0;
    }
    __syncthreads();
    // kept points whose circle reaches this tile
    for (int k = threadIdx.x; k < n_kept; k += kTrkT) {
        const int2 c = j.kept_pix[k];
        if (c.x + r >= x0 && c.x - r < x0 + kTrkTW && c.y + r >= y0 && c.y - r < y0 + kTrkTH) s_list[atomicAdd(&s_nlist, 1)] = c;
    }
    // Sobel at every cell the box sums of this tile read; a cell outside the image holds the derivative of its REFLECT_101 image
    for (int k = threadIdx.x; k < (kTrkTH + 2) * (kTrkTW + 2); k += kTrkT) {
        const int ly = k / (kTrkTW + 2), lx = k - ly * (kTrkTW + 2);
        const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
        int dx = 0, dy = 0;
        if (gy >= -1 && gy <= h && gx >= -1 && gx <= w) {
            const int qy = trk_reflect(gy, h), qx = trk_reflect(gx, w);
            const int ya = trk_reflect(qy - 1, h) - (y0 - 2), yb = qy - (y0 - 2), yc = trk_reflect(qy + 1, h) - (y0 - 2);
            const int xa = trk_reflect(qx - 1, w) - (x0 - 2), xb = qx - (x0 - 2), xc = trk_reflect(qx + 1, w) - (x0 - 2);
            dx = (s_img[ya][xc] + 2 * s_img[yb][xc] + s_img[yc][xc]) - (s_img[ya][xa] + 2 * s_img[yb][xa] + s_img[yc][xa]);
            dy = (s_img[yc][xa] + 2 * s_img[yc][xb] + s_img[yc][xc]) - (s_img[ya][xa] + 2 * s_img[ya][xb] + s_img[ya][xc]);
        }
        s_dx[ly][lx] = (short)dx; s_dy[ly][lx] = (short)dy;
    }
    __syncthreads();
    const int nlist = s_nlist;
    const double sc2 = (1.0 / (12.0 * 255.0)) * (1.0 / (12.0 * 255.0));
    unsigned int best = 0u;
    for (int k = threadIdx.x; k < kTrkTH * kTrkTW; k += kTrkT) {
        const int ly = k / kTrkTW, lx = k - ly * kTrkTW;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= h || gx >= w) continue;
        int sxx = 0, sxy = 0, syy = 0;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) {
                const int dx = s_dx[ly + a][lx + b], dy = s_dy[ly + a][lx + b];
                sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
            }
        const double A = (double)sxx * sc2, B = (double)sxy * sc2, C = (double)syy * sc2;
        const double d = A - C;
        const float v = (float)(0.5 * (A + C) - sqrt((0.25 * d) * d + B * B));
        j.resp[(size_t)gy * w + gx] = v;
        if (v > 0.f) {
            bool masked = false;
            for (int q = 0; q < nlist; q++) masked = masked || trk_in_circle(s_hw, r, gx - s_list[q].x, gy - s_list[q].y);
            if (!masked) best = max(best, __float_as_uint(v));
        }
    }
    best = wave_max_u32_uniform(best);
    if (lane_id() == 0 && best) atomicMax(&j.st->max_bits, best);
}

__global__ __launch_bounds__(kTrkT) void k_trk_nms(const TrkJob *jobs)
{
    const TrkJob &j = jobs[blockIdx.y];
    const TrkState *st = j.st;
    if (st->quota <= 0) return;
    const int w = j.w, h = j.h, iw = w - 2, n_int = iw * (h - 2);
    const float thr = (float)((double)__uint_as_float(st->max_bits) * 0.01);
    const int r = j.min_dist, n_kept = st->n_kept;
    for (int k = blockIdx.x * kTrkT + threadIdx.x; k < n_int; k += gridDim.x * kTrkT) {
        const int y = 1 + k / iw, x = 1 + k % iw;
        const float *p = j.resp + (size_t)y * w + x;
        const float v = p[0];
        if (!(v > thr)) continue;
        const float m = fmaxf(fmaxf(fmaxf(p[-w - 1], p[-w]), fmaxf(p[-w + 1], p[-1])), fmaxf(fmaxf(p[1], p[w - 1]), fmaxf(p[w], p[w + 1])));
        if (m > v) continue;
        bool masked = false;
        for (int q = 0; q < n_kept && !masked; q++) { const int2 c = j.kept_pix[q]; masked = trk_in_circle(j.hw, r, x - c.x, y - c.y); }
        if (masked) continue;
        const int slot = atomicAdd(&j.st->n_cand, 1);
        j.cand[slot] = ((unsigned long long)__float_as_uint(v) << 32) | (0xFFFFFFFFu - (unsigned int)(y * w + x));     // larger key: stronger, then lower pixel index
    }
}

// one workgroup per stream: the strongest live key is selected, every lane then kills the keys of its own candidates closer than
// MIN_DIST to it (the selected one included) -- the sequential greedy pass of cv::goodFeaturesToTrack over the sorted list
__global__ __launch_bounds__(kTrkT) void k_trk_select(const TrkJob *jobs)
{
    __shared__ unsigned long long s_best[kTrkT / kWave];
    const TrkJob &j = jobs[blockIdx.x];
    TrkState *st = j.st;
    const int quota = st->quota, n_cand = st->n_cand, w = j.w;
    if (quota <= 0) return;
    const long long r2 = (long long)j.min_dist * j.min_dist;
    int n_sel = 0;
    while (n_sel < quota) {
        unsigned long long best = 0ull;
        for (int k = threadIdx.x; k < n_cand; k += kTrkT) { const unsigned long long key = j.cand[k]; best = key > best ? key : best; }
        best = wave_max_key_uniform(best);
        __syncthreads();
        if (lane_id() == 0) s_best[threadIdx.x >> 6] = best;
        __syncthreads();
        best = s_best[0];
#pragma unroll
        for (int q = 1; q < kTrkT / kWave; q++) best = s_best[q] > best ? s_best[q] : best;
        if (best == 0ull) break;
        const int pix = (int)(0xFFFFFFFFu - (unsigned int)best);
        const int sy = pix / w, sx = pix - sy * w;
        if (threadIdx.x == 0) j.new_pts[n_sel] = make_int2(sx, sy);
        n_sel++;
        for (int k = threadIdx.x; k < n_cand; k += kTrkT) {
            const unsigned long long key = j.cand[k];
            if (key == 0ull) continue;
            const int p = (int)(0xFFFFFFFFu - (unsigned int)key);
            const long long dy = p / w - sy, dx = p % w - sx;
            if (dx * dx + dy * dy < r2) j.cand[k] = 0ull;
        }
    }
    if (threadIdx.x == 0) st->n_new = n_sel;
}

__device__ __forceinline__ float2 trk_lift(const ColourCam &c, float2 p)      // PinholeCamera::liftProjective, PinholeCamera.cc:450-510
{
    const double mx_d = c.ik11 * (double)p.x + c.ik13, my_d = c.ik22 * (double)p.y + c.ik23;
    double mx_u = mx_d, my_u = my_d;
    if (c.distort) {
        for (int it = 0; it < 8; it++) {
            double dx, dy;
            col_distortion(c, mx_u, my_u, dx, dy);
            mx_u = mx_d - dx; my_u = my_d - dy;
        }
    }
    return make_float2((float)mx_u, (float)my_u);
}

__global__ __launch_bounds__(kTrkMaxPts) void k_trk_finish(const TrkJob *jobs)
{
    const TrkJob &j = jobs[blockIdx.x];
    TrkState *st = j.st;
    const int i = threadIdx.x, n_kept = st->n_kept, n_new = st->n_new, n_id = st->n_id, n = n_kept + n_new;
    __syncthreads();      // every wave has read the counters before thread 0 overwrites them below
    if (i < n) {
        float2 p; int id, cnt;
        const bool hp = i < n_kept;          // a survivor is in prev_un_pts_map, a new corner is not (:110-121)
        if (hp) { p = j.pts[i]; id = j.ids[i]; cnt = j.cnt[i]; }
        else {
            const int2 c = j.new_pts[i - n_kept];
            p = make_float2((float)c.x, (float)c.y); id = n_id + (i - n_kept); cnt = 1;
            j.pts[i] = p; j.ids[i] = id; j.cnt[i] = cnt;
        }
        const float2 un = trk_lift(j.cam, p);
        lmono_track_record rec;
        rec.id = id; rec.x_n = un.x; rec.y_n = un.y; rec.u = p.x; rec.v = p.y; rec.vx = 0.f; rec.vy = 0.f; rec.track_cnt = cnt;
        if (hp) {
            const float2 o = j.un[i];
            rec.vx = (float)((double)(un.x - o.x) / j.dt);
            rec.vy = (float)((double)(un.y - o.y) / j.dt);
        }
        j.un[i] = un;
        j.rec[i] = rec;
    }
    if (i == 0) { st->n = n; st->n_id = n_id + n_new; *j.n_out = n; }
}

} // namespace lmono

#include "track_reject.hip"
