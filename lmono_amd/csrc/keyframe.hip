// keyframe.hip -- keyframe descriptor kernels (gfx950, wave64): KeyFrame::computeBRIEFPoint / computeWindowBRIEFPoint / searchByBRIEFDes
// (mono_lidar_mapping/src/loop_detection/KeyFrame.cc:172-267) with DVision's BRIEF::compute (src/loop_detection/DVision/BRIEF.cpp:39-106).
// DESIGN.md 6f holds the written definition these kernels and tests/keyframe_ref.py implement; everything but the normalised keypoints is
// integer arithmetic.  FAST (item 2) and the blur (item 3) are definitions of this project: parity with cv::FAST / cv::GaussianBlur is unpinned.
//   k_kf_blur             BGR2GRAY or copy on load, 9 x 9 Gaussian (sigma 2) in 1/256, REFLECT_101: tile + 4-pixel halo in LDS, both passes in LDS
//   k_kf_fast_score       FAST-9/16 score per pixel: tile + 3-pixel halo in LDS, brighter / darker masks with a rotate-and-AND run test, the
//                         arc minima only for the survivors
//   k_kf_fast_nms_count   3 x 3 strict non-maximum suppression, kept corners per image row (one wave per row)
//   k_kf_fast_nms_scan    exclusive prefix over the rows, the total, the capacity check (one workgroup per stream)
//   k_kf_fast_nms_write   stable row-major write of the keypoints + liftProjective (KeyFrame.cc:202-209)
//   k_kf_brief            one wave per point (FAST keypoints, then window points), four tests per lane, words by ballot
//   k_kf_match            searchInAera for every (window descriptor, old keyframe): a workgroup keeps the window descriptors in registers and
//                         streams a 256-descriptor share of one old keyframe past them through LDS; key = dist << 16 | index, atomicMin
//   k_kf_match_finish     the < 80 gate, the gather of the matched points, the count per old keyframe
#pragma once
#include "common.hpp"
#include "colour.hip"
#include "track.hip"

namespace lmono {

constexpr int kKfT = 256;
constexpr int kKfTW = 64, kKfTH = 16;           // image tile
constexpr int kKfMaxWin = LMONO_TRACK_MAX_POINTS;
constexpr int kKfShare = 256;                   // old descriptors per workgroup of k_kf_match
constexpr unsigned int kKfNoMatch = (128u << 16) | 0xFFFFu;

struct KfJob {
    int w, h, format, thr, max_kp, n_win;
    ColourCam cam;
    const unsigned char *src;            // the frame: [h][w] grey or [h][w][3] BGR
    unsigned char *blur, *score;         // work images of the store
    int *row_cnt, *row_off;              // [h]
    int *res;                            // [2]: corners found, 1 when they exceed max_kp (nothing is written then)
    int *n_kp;                           // the slot's keypoint count
    float2 *kp, *norm;                   // the slot's arrays
    uint32_t *desc;
    const float2 *win_uv;
    uint32_t *win_desc;
    const char4 *pat;                    // [256] (x1, y1, x2, y2)
};

__device__ __forceinline__ int kf_grey(const KfJob &j, int x, int y)
{
    const size_t i = (size_t)y * j.w + x;
    if (j.format == 0) return j.src[i];
    return trk_bgr_to_grey(j.src[3 * i], j.src[3 * i + 1], j.src[3 * i + 2]);
}

__global__ __launch_bounds__(kKfT) void k_kf_blur(const KfJob *jobs)
{
    __shared__ unsigned char s_img[kKfTH + 8][kKfTW + 8];
    __shared__ unsigned short s_row[kKfTH + 8][kKfTW];
    const KfJob &j = jobs[blockIdx.y];
    const int w = j.w, h = j.h, tiles_x = (w + kKfTW - 1) / kKfTW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * kKfTW, y0 = ty * kKfTH;
    if (y0 >= h) return;
    for (int k = threadIdx.x; k < (kKfTH + 8) * (kKfTW + 8); k += kKfT) {
        const int ly = k / (kKfTW + 8), lx = k - ly * (kKfTW + 8);
        s_img[ly][lx] = (unsigned char)kf_grey(j, trk_reflect(x0 - 4 + lx, w), trk_reflect(y0 - 4 + ly, h));
    }
    __syncthreads();
    for (int k = threadIdx.x; k < (kKfTH + 8) * kKfTW; k += kKfT) {
        const int ly = k / kKfTW, lx = k - ly * kKfTW;
        const unsigned char *p = &s_img[ly][lx];
        s_row[ly][lx] = (unsigned short)(7 * (p[0] + p[8]) + 17 * (p[1] + p[7]) + 32 * (p[2] + p[6]) + 46 * (p[3] + p[5]) + 52 * p[4]);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kKfTH * kKfTW; k += kKfT) {
        const int ly = k / kKfTW, lx = k - ly * kKfTW;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx >= w || gy >= h) continue;
        const int sum = 7 * (s_row[ly][lx] + s_row[ly + 8][lx]) + 17 * (s_row[ly + 1][lx] + s_row[ly + 7][lx]) + 32 * (s_row[ly + 2][lx] + s_row[ly + 6][lx]) +
                        46 * (s_row[ly + 3][lx] + s_row[ly + 5][lx]) + 52 * s_row[ly + 4][lx];
        j.blur[(size_t)gy * w + gx] = (unsigned char)((sum + 32768) >> 16);
    }
}

// bit i of the result: positions i .. i + 8 (circular, 16 positions) of m are all set -- a run of 9 starts at i
__device__ __forceinline__ unsigned int kf_run9(unsigned int m)
{
    unsigned int mm = m | (m << 16);
    unsigned int r = mm & (mm >> 1);          // runs of 2 (bits 0..15 valid while the doubled word is refreshed)
    r = (r & 0xFFFFu) | (r << 16);
    r &= r >> 2;                              // 4
    r = (r & 0xFFFFu) | (r << 16);
    r &= r >> 4;                              // 8
    r = (r & 0xFFFFu) | (r << 16);
    r &= mm >> 8;                             // 9
    return r & 0xFFFFu;
}

__global__ __launch_bounds__(kKfT) void k_kf_fast_score(const KfJob *jobs)
{
    __shared__ unsigned char s_img[kKfTH + 6][kKfTW + 6];
    const KfJob &j = jobs[blockIdx.y];
    const int w = j.w, h = j.h, tiles_x = (w + kKfTW - 1) / kKfTW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * kKfTW, y0 = ty * kKfTH;
    if (y0 >= h) return;
    for (int k = threadIdx.x; k < (kKfTH + 6) * (kKfTW + 6); k += kKfT) {
        const int ly = k / (kKfTW + 6), lx = k - ly * (kKfTW + 6);
        const int gx = x0 - 3 + lx, gy = y0 - 3 + ly;
        s_img[ly][lx] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? (unsigned char)kf_grey(j, gx, gy) : (unsigned char)0;
    }
    __syncthreads();
    const int t = j.thr;
    for (int k = threadIdx.x; k < kKfTH * kKfTW; k += kKfT) {
        const int ly = k / kKfTW, lx = k - ly * kKfTW;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx >= w || gy >= h) continue;
        int score = 0;
        if (gx >= 3 && gx < w - 3 && gy >= 3 && gy < h - 3) {
            const unsigned char *c = &s_img[ly + 3][lx + 3];
            const int v = c[0];
            constexpr int kRow = kKfTW + 6;
            const int d[16] = { v - c[3 * kRow], v - c[3 * kRow + 1], v - c[2 * kRow + 2], v - c[kRow + 3], v - c[3], v - c[-kRow + 3], v - c[-2 * kRow + 2], v - c[-3 * kRow + 1],
                                v - c[-3 * kRow], v - c[-3 * kRow - 1], v - c[-2 * kRow - 2], v - c[-kRow - 3], v - c[-3], v - c[kRow - 3], v - c[2 * kRow - 2], v - c[3 * kRow - 1] };
            unsigned int bright = 0u, dark = 0u;
#pragma unroll
            for (int q = 0; q < 16; q++) { bright |= (d[q] > t ? 1u : 0u) << q; dark |= (-d[q] > t ? 1u : 0u) << q; }
            if (kf_run9(bright) | kf_run9(dark)) {
                int best = -256;
#pragma unroll
                for (int s = 0; s < 16; s++) {
                    int lo = d[s], hi = d[s];
#pragma unroll
                    for (int q = 1; q < 9; q++) { lo = min(lo, d[(s + q) & 15]); hi = max(hi, d[(s + q) & 15]); }
                    best = max(best, max(lo, -hi));
                }
                score = best - 1;
            }
        }
        j.score[(size_t)gy * w + gx] = (unsigned char)score;
    }
}

// score > 0 implies 3 <= x < w - 3 and 3 <= y < h - 3, so every neighbour exists
__device__ __forceinline__ bool kf_kept(const unsigned char *score, int w, int x, int y)
{
    const unsigned char *p = score + (size_t)y * w + x;
    const int s = p[0];
    if (s == 0) return false;
    return s > p[-w - 1] && s > p[-w] && s > p[-w + 1] && s > p[-1] && s > p[1] && s > p[w - 1] && s > p[w] && s > p[w + 1];
}

__global__ __launch_bounds__(kKfT) void k_kf_fast_nms_count(const KfJob *jobs)
{
    const KfJob &j = jobs[blockIdx.y];
    const int y = blockIdx.x * (kKfT / kWave) + (threadIdx.x >> 6);
    if (y >= j.h) return;
    int n = 0;
    if (y >= 3 && y < j.h - 3)
        for (int x = 3 + lane_id(); x < j.w - 3; x += kWave) n += kf_kept(j.score, j.w, x, y) ? 1 : 0;
    n = wave_sum_i(n);
    if (lane_id() == 0) j.row_cnt[y] = n;
}

__global__ __launch_bounds__(kKfT) void k_kf_fast_nms_scan(const KfJob *jobs)
{
    __shared__ int s_sum[kKfT];
    const KfJob &j = jobs[blockIdx.x];
    const int per = (j.h + kKfT - 1) / kKfT, r0 = threadIdx.x * per, r1 = min(r0 + per, j.h);
    int sum = 0;
    for (int r = r0; r < r1; r++) sum += j.row_cnt[r];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    int base = 0, total = 0;
    for (int k = 0; k < kKfT; k++) { const int v = s_sum[k]; total += v; base += k < (int)threadIdx.x ? v : 0; }
    for (int r = r0; r < r1; r++) { j.row_off[r] = base; base += j.row_cnt[r]; }
    if (threadIdx.x == 0) {
        const int over = total > j.max_kp ? 1 : 0;
        j.res[0] = total; j.res[1] = over;
        if (!over) *j.n_kp = total;
    }
}

__global__ __launch_bounds__(kKfT) void k_kf_fast_nms_write(const KfJob *jobs)
{
    const KfJob &j = jobs[blockIdx.y];
    const int y = blockIdx.x * (kKfT / kWave) + (threadIdx.x >> 6), lane = lane_id();
    if (y < 3 || y >= j.h - 3 || j.res[1]) return;
    if (j.row_cnt[y] == 0) return;
    int at = j.row_off[y];
    for (int xb = 3; xb < j.w - 3; xb += kWave) {
        const int x = xb + lane;
        const bool keep = x < j.w - 3 && kf_kept(j.score, j.w, x, y);
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int slot = at + __popcll(m & ((1ull << lane) - 1ull));
            const float2 p = make_float2((float)x, (float)y);
            j.kp[slot] = p;
            j.norm[slot] = trk_lift(j.cam, p);
        }
        at += __popcll(m);
    }
}

// point p < n_kp: FAST keypoint p; n_kp <= p < n_kp + n_win: window point p - n_kp.  Lane l owns tests l, l + 64, l + 128, l + 192 of every
// point, so the ballot of round k is words 2 k and 2 k + 1 of the descriptor.
__global__ __launch_bounds__(kKfT) void k_kf_brief(const KfJob *jobs)
{
    const KfJob &j = jobs[blockIdx.y];
    if (j.res[1]) return;
    const int lane = lane_id(), n_kp = j.res[0], n = n_kp + j.n_win;
    const int wave = blockIdx.x * (kKfT / kWave) + (threadIdx.x >> 6), n_waves = gridDim.x * (kKfT / kWave);
    if (wave >= n) return;
    char4 pat[4];
#pragma unroll
    for (int k = 0; k < 4; k++) pat[k] = j.pat[lane + 64 * k];
    const float fw = (float)j.w, fh = (float)j.h;
    for (int p = wave; p < n; p += n_waves) {
        const float2 pt = p < n_kp ? j.kp[p] : j.win_uv[p - n_kp];
        uint32_t *out = p < n_kp ? j.desc + 8 * (size_t)p : j.win_desc + 8 * (size_t)(p - n_kp);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            // (int)(pt + offset) lies in [0, n) exactly when the fp32 sum lies in (-1, n): the conversion truncates toward zero
            const float x1 = pt.x + (float)pat[k].x, y1 = pt.y + (float)pat[k].y, x2 = pt.x + (float)pat[k].z, y2 = pt.y + (float)pat[k].w;
            bool bit = x1 > -1.f && x1 < fw && y1 > -1.f && y1 < fh && x2 > -1.f && x2 < fw && y2 > -1.f && y2 < fh;
            if (bit) bit = j.blur[(size_t)(int)y1 * j.w + (int)x1] < j.blur[(size_t)(int)y2 * j.w + (int)x2];
            const unsigned long long m = __ballot(bit);
            if (lane == 0) { out[2 * k] = (uint32_t)m; out[2 * k + 1] = (uint32_t)(m >> 32); }
        }
    }
}

struct KfMatchJob {
    const uint32_t *cur_desc;            // [n_win][8] window descriptors of the current keyframe
    int n_win, n_old;
    const int *old_slot;                 // [n_old] slots of the old keyframes
    const int *n_kp;                     // [slots]
    const uint32_t *desc;                // [slots][max_kp][8]
    const float2 *kp, *norm;             // [slots][max_kp]
    int max_kp;
    unsigned int *keys;                  // [n_old][n_win], preset to kKfNoMatch
    unsigned char *status;               // outputs [n_old][n_win]
    int *index, *dist;
    float2 *old_uv, *old_norm;
    int *counts;                         // [n_old]
};

__device__ __forceinline__ int kf_hamming(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1)
{
    return __popcll(((unsigned long long)(a0.y ^ b0.y) << 32) | (a0.x ^ b0.x)) + __popcll(((unsigned long long)(a0.w ^ b0.w) << 32) | (a0.z ^ b0.z)) +
           __popcll(((unsigned long long)(a1.y ^ b1.y) << 32) | (a1.x ^ b1.x)) + __popcll(((unsigned long long)(a1.w ^ b1.w) << 32) | (a1.z ^ b1.z));
}

// grid (shares, old keyframes); thread t owns window descriptors t and t + 256
__global__ __launch_bounds__(kKfT) void k_kf_match(KfMatchJob mj)
{
    __shared__ uint4 s_old[kKfShare][2];
    const int o = blockIdx.y, slot = mj.old_slot[o];
    const int n_old_kp = mj.n_kp[slot], i0 = blockIdx.x * kKfShare, n_here = min(kKfShare, n_old_kp - i0);
    if (n_here <= 0) return;
    const uint4 *od = (const uint4 *)(mj.desc + ((size_t)slot * mj.max_kp + i0) * 8);
    for (int k = threadIdx.x; k < 2 * n_here; k += kKfT) s_old[k >> 1][k & 1] = od[k];
    const int c0 = threadIdx.x, c1 = threadIdx.x + kKfT;
    const bool has0 = c0 < mj.n_win, has1 = c1 < mj.n_win;
    const uint4 *cd = (const uint4 *)mj.cur_desc;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    const uint4 a00 = has0 ? cd[2 * c0] : z, a01 = has0 ? cd[2 * c0 + 1] : z, a10 = has1 ? cd[2 * c1] : z, a11 = has1 ? cd[2 * c1 + 1] : z;
    __syncthreads();
    unsigned int best0 = kKfNoMatch, best1 = kKfNoMatch;
    const bool second = mj.n_win > kKfT;         // uniform
    for (int i = 0; i < n_here; i++) {
        const uint4 b0 = s_old[i][0], b1 = s_old[i][1];
        const unsigned int idx = (unsigned int)(i0 + i);
        best0 = min(best0, ((unsigned int)kf_hamming(a00, a01, b0, b1) << 16) | idx);
        if (second) best1 = min(best1, ((unsigned int)kf_hamming(a10, a11, b0, b1) << 16) | idx);
    }
    unsigned int *keys = mj.keys + (size_t)o * mj.n_win;
    if (has0 && best0 < kKfNoMatch) atomicMin(&keys[c0], best0);
    if (has1 && best1 < kKfNoMatch) atomicMin(&keys[c1], best1);
}

__global__ __launch_bounds__(kKfMaxWin) void k_kf_match_finish(KfMatchJob mj)
{
    __shared__ int s_count;
    const int o = blockIdx.x, c = threadIdx.x, slot = mj.old_slot[o];
    if (c == 0) s_count = 0;
    __syncthreads();
    if (c < mj.n_win) {
        const size_t at = (size_t)o * mj.n_win + c;
        const unsigned int key = mj.keys[at];
        // a distance of exactly 128 orders below the preset key but is no candidate: the scan starts from 128 with a strict <
        const int dist = (int)(key >> 16), idx = dist >= 128 ? -1 : (int)(key & 0xFFFFu);
        const bool ok = idx >= 0 && dist < 80;
        float2 uv = make_float2(0.f, 0.f), nm = uv;
        if (ok) { uv = mj.kp[(size_t)slot * mj.max_kp + idx]; nm = mj.norm[(size_t)slot * mj.max_kp + idx]; atomicAdd(&s_count, 1); }
        mj.status[at] = ok ? 1 : 0; mj.index[at] = idx; mj.dist[at] = dist; mj.old_uv[at] = uv; mj.old_norm[at] = nm;
    }
    __syncthreads();
    if (c == 0) mj.counts[o] = s_count;
}

} // namespace lmono
