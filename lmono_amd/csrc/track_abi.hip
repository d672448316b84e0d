// track_abi.hip -- C ABI of the image feature tracker (included by lmono_hip.hip after lmono_ctx is defined)
#pragma once
#include "track.hip"

struct lmono_tracker {
    lmono_ctx *ctx = nullptr;
    TrkJob job{};                        // the stream's device pointers and constants; per-frame fields are filled per call
    TrkPyr pyr[2]{};
    int cur = 0;                         // pyr[cur] holds the last frame
    int frames = 0;
    double prev_time = 0.0;
    bool stale = false;                  // a frame failed half way: the device counters are not trustworthy until lmono_tracker_reset
    float2 *lk_pts = nullptr;            // staging of the diagnostic LK call
    unsigned char *image = nullptr;      // staging of the host-buffer entry ([h][w][3])
    // rejectWithF (lmono_tracker_set_reject_f): parameters, device outputs, the last frame's stats / F on the host
    bool rej_on = false, rej_ran = false;
    lmono_reject_f rej{};
    unsigned char *rej_st = nullptr;
    int *rej_stats = nullptr;
    double *rej_F = nullptr;
    float2 *rej_prev = nullptr, *rej_cur = nullptr;      // staging of the diagnostic call
    int32_t last_stats[4] = { -1, -1, -1, -1 };
    double last_F[9] = {};
    DevOwner mem;
    // job table + counts of a batch led by this tracker
    TrkJob *jobs = nullptr;
    int *counts = nullptr;
    int jobs_cap = 0;
};

extern "C" void lmono_tracker_destroy(lmono_tracker *t) { delete t; }

extern "C" int lmono_tracker_reset(lmono_ctx *c, lmono_tracker *t)
{
    if (!c || !t || t->ctx != c) return LMONO_EINVAL;
    HIP_TRY(c, hipMemsetAsync(t->job.st, 0, sizeof(TrkState), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    t->frames = 0; t->prev_time = 0.0; t->stale = false; t->rej_ran = false;
    return LMONO_OK;
}

extern "C" lmono_tracker *lmono_tracker_create(lmono_ctx *c, const lmono_camera *cam, int max_cnt, int min_dist, int flags)
{
    if (!c) return nullptr;
    if (!cam || cam->width <= kTrkWin || cam->height <= kTrkWin || cam->width > 8192 || cam->height > 8192 || max_cnt < 1 || max_cnt > kTrkMaxPts ||
        min_dist < 1 || min_dist > kTrkMaxRadius || flags != 0 || !(cam->fx != 0.0) || !(cam->fy != 0.0)) {
        c->err = (flags & LMONO_TRACK_REJECT_F) ? "lmono_tracker_create: rejectWithF is not switched on by flags (flags must be 0): use lmono_tracker_set_reject_f"
                                                : "lmono_tracker_create: bad camera / limits (image sides 22..8192, 1 <= max_cnt <= 512, 1 <= min_dist <= 128, flags 0)";
        return nullptr;
    }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return nullptr; }
    lmono_tracker *t = new lmono_tracker();
    t->ctx = c;
    TrkJob &j = t->job;
    j.w = cam->width; j.h = cam->height; j.max_cnt = max_cnt; j.min_dist = min_dist; j.lk_n = -1;
    colour_cam_from(*cam, j.cam);
    {   // rows of cv::circle(mask, pt, MIN_DIST, 0, -1): the filled midpoint circle of OpenCV's drawing.cpp
        int err = 0, dx = min_dist, dy = 0, plus = 1, minus = 2 * min_dist - 1;
        for (int i = 0; i <= kTrkMaxRadius; i++) j.hw[i] = 0;
        while (dx >= dy) {
            j.hw[dy] = std::max(j.hw[dy], dx);
            j.hw[dx] = std::max(j.hw[dx], dy);
            dy++; err += plus; plus += 2;
            if (err > 0) { err -= minus; dx--; minus -= 2; }
        }
    }
    // cv::buildOpticalFlowPyramid: a level exists while both of its sides exceed the window
    int lw[kTrkLevels], lh[kTrkLevels];
    lw[0] = j.w; lh[0] = j.h; j.n_levels = 1;
    while (j.n_levels < kTrkLevels) {
        const int w2 = (lw[j.n_levels - 1] + 1) / 2, h2 = (lh[j.n_levels - 1] + 1) / 2;
        if (w2 <= kTrkWin || h2 <= kTrkWin) break;
        lw[j.n_levels] = w2; lh[j.n_levels] = h2; j.n_levels++;
    }
    const size_t np = (size_t)j.w * j.h;
    DevOwner &m = t->mem;
    bool ok = true;
    for (int b = 0; b < 2 && ok; b++)
        for (int l = 0; l < j.n_levels && ok; l++) {
            TrkLevel &L = t->pyr[b].lv[l];
            L.w = lw[l]; L.h = lh[l];
            ok = m.alloc(L.img, (size_t)L.w * L.h) && m.alloc(L.dx, (size_t)L.w * L.h) && m.alloc(L.dy, (size_t)L.w * L.h);
        }
    ok = ok && m.alloc(j.st, 1) && m.alloc(j.pts, kTrkMaxPts) && m.alloc(j.un, kTrkMaxPts) && m.alloc(j.ids, kTrkMaxPts) && m.alloc(j.cnt, kTrkMaxPts) &&
         m.alloc(j.cur_pts, kTrkMaxPts) && m.alloc(j.rev_pts, kTrkMaxPts) && m.alloc(j.st_f, kTrkMaxPts) && m.alloc(j.st_b, kTrkMaxPts) &&
         m.alloc(j.kept_pix, kTrkMaxPts) && m.alloc(j.resp, np) && m.alloc(j.cand, np) && m.alloc(j.new_pts, kTrkMaxPts) &&
         m.alloc(j.rec, kTrkMaxPts) && m.alloc(t->lk_pts, kTrkMaxPts) && m.alloc(t->image, np * 3) &&
         m.alloc(t->rej_st, kTrkMaxPts) && m.alloc(t->rej_stats, 4) && m.alloc(t->rej_F, 9) && m.alloc(t->rej_prev, kTrkMaxPts) && m.alloc(t->rej_cur, kTrkMaxPts);
    ok = ok && hipMemset(j.st, 0, sizeof(TrkState)) == hipSuccess && hipMemset(j.resp, 0, np * sizeof(float)) == hipSuccess;
    if (!ok) { c->err = "lmono_tracker_create: device allocation failed"; lmono_tracker_destroy(t); return nullptr; }
    return t;
}

// the job's rejectWithF fields from the tracker's parameters; n >= 0: the diagnostic call on n staged pairs
static void trk_reject_job(const lmono_tracker *t, TrkJob &j, int n, uint32_t frame_key)
{
    j.rej_st = t->rej_st; j.rej_stats = t->rej_stats; j.rej_F = t->rej_F;
    j.rej_thr2 = t->rej.f_threshold * t->rej.f_threshold; j.rej_dis = t->rej.f_dis; j.rej_focal = t->rej.focal_length;
    j.rej_nhyp = t->rej.n_hyp; j.rej_seed = t->rej.seed; j.rej_key = frame_key; j.rej_n = n;
    j.rej_prev = t->rej_prev; j.rej_cur = t->rej_cur;
}

extern "C" int lmono_tracker_set_reject_f(lmono_ctx *c, lmono_tracker *t, const lmono_reject_f *p)
{
    if (!c || !t || t->ctx != c) return LMONO_EINVAL;
    if (!p) { t->rej_on = false; return LMONO_OK; }
    if (!(p->f_threshold > 0.0) || !std::isfinite(p->f_threshold) || !(p->f_dis > 0.0) || !std::isfinite(p->f_dis) || !(p->focal_length >= 0.0) ||
        !std::isfinite(p->focal_length) || p->n_hyp < 0 || p->n_hyp > kRejMaxHyp) {
        c->err = "lmono_tracker_set_reject_f: f_threshold and f_dis must be finite and > 0, focal_length finite and >= 0, 0 <= n_hyp <= 1024";
        return LMONO_EINVAL;
    }
    t->rej = *p;
    if (t->rej.focal_length == 0.0) t->rej.focal_length = 460.0;      // FOCAL_LENGTH, parameter.h:50
    if (t->rej.n_hyp == 0) t->rej.n_hyp = 256;
    t->rej_on = true;
    return LMONO_OK;
}

extern "C" int lmono_tracker_reject_stats(lmono_ctx *c, lmono_tracker *t, int32_t *stats, double *F)
{
    if (!c || !t || t->ctx != c) return LMONO_EINVAL;
    for (int k = 0; k < 4 && stats; k++) stats[k] = t->rej_ran ? t->last_stats[k] : -1;
    for (int k = 0; k < 9 && F; k++) F[k] = t->rej_ran ? t->last_F[k] : 0.0;
    return LMONO_OK;
}

static int trk_job_table(lmono_ctx *c, lmono_tracker *lead, int n_streams, const char *who)
{
    if (!job_table(lead->mem, lead->jobs, lead->counts, lead->jobs_cap, n_streams, 1)) { c->err = std::string(who) + ": job table allocation failed"; return LMONO_ENOMEM; }
    return LMONO_OK;
}

static inline unsigned trk_blocks(size_t n) { return (unsigned)std::min<size_t>((n + kTrkT - 1) / kTrkT, 4096); }

extern "C" int lmono_tracker_track_batch(lmono_ctx *c, int n_streams, lmono_tracker *const *trks, const double *times, const uint8_t *const *image_d, int format,
                                         lmono_track_record *const *records_out, const int *caps, int *n_out)
{
    if (!c || n_streams <= 0 || !trks || !times || !image_d || !n_out || (format != LMONO_TRACK_GREY8 && format != LMONO_TRACK_BGR8)) return LMONO_EINVAL;
    for (int s = 0; s < n_streams; s++) {
        const int fault = batch_handle_fault(c, s, trks);
        if (fault == kHandleForeign || !image_d[s]) { c->err = "lmono_tracker_track_batch: bad stream arguments"; return LMONO_EINVAL; }
        if (trks[s]->stale) { c->err = "lmono_tracker_track_batch: an earlier frame of this tracker failed half way; call lmono_tracker_reset"; return LMONO_EINVAL; }
        if (fault == kHandleRepeated) { c->err = "lmono_tracker_track_batch: trackers must be distinct"; return LMONO_EINVAL; }
        if (records_out && records_out[s] && (!caps || caps[s] < trks[s]->job.max_cnt)) { c->err = "lmono_tracker_track_batch: record capacity below max_cnt"; return LMONO_ECAPACITY; }
    }
    lmono_tracker *lead = trks[0];
    if (int rc = trk_job_table(c, lead, n_streams, "lmono_tracker_track_batch")) return rc;
    std::vector<TrkJob> jobs((size_t)n_streams);
    size_t max_np = 0; int max_levels = 1, max_cnt = 1, max_tiles = 1;
    bool any_reject = false;
    for (int s = 0; s < n_streams; s++) {
        lmono_tracker *t = trks[s];
        TrkJob &j = jobs[(size_t)s];
        j = t->job;
        j.cur = t->pyr[t->cur ^ 1]; j.prev = t->pyr[t->cur];   // prev_img = cur_img (:359) by pointer swap, committed when the frame has succeeded
        j.src = image_d[s]; j.format = format; j.lk_n = -1;
        j.dt = times[s] - t->prev_time;
        j.n_out = lead->counts + s;
        if (t->rej_on) { trk_reject_job(t, j, -1, (uint32_t)t->frames); any_reject = true; }
        max_np = std::max(max_np, (size_t)j.w * j.h);
        max_levels = std::max(max_levels, j.n_levels); max_cnt = std::max(max_cnt, j.max_cnt);
        max_tiles = std::max(max_tiles, ((j.w + kTrkTW - 1) / kTrkTW) * ((j.h + kTrkTH - 1) / kTrkTH));
    }
    const unsigned ns = (unsigned)n_streams;
    for (int s = 0; s < n_streams; s++) trks[s]->stale = true;     // until the last step below has succeeded
    HIP_TRY(c, hipMemcpyAsync(lead->jobs, jobs.data(), sizeof(TrkJob) * (size_t)n_streams, hipMemcpyHostToDevice, c->stream));
    k_trk_grey<<<dim3(trk_blocks(max_np), ns), kTrkT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_trk_grey")) return rc;
    for (int l = 1; l < max_levels; l++) {
        k_trk_pyrdown<<<dim3(trk_blocks(max_np >> (2 * l - 1)), ns), kTrkT, 0, c->stream>>>(lead->jobs, l);
        if (int rc = check_launch(c, "k_trk_pyrdown")) return rc;
    }
    for (int l = 0; l < max_levels; l++) {
        k_trk_scharr<<<dim3(trk_blocks(l ? max_np >> (2 * l - 1) : max_np), ns), kTrkT, 0, c->stream>>>(lead->jobs, l);
        if (int rc = check_launch(c, "k_trk_scharr")) return rc;
    }
    const unsigned lk_blocks = (unsigned)((max_cnt + kTrkT / kWave - 1) / (kTrkT / kWave));
    k_trk_lk<<<dim3(lk_blocks, ns), kTrkT, 0, c->stream>>>(lead->jobs, 0);
    if (int rc = check_launch(c, "k_trk_lk")) return rc;
    k_trk_lk<<<dim3(lk_blocks, ns), kTrkT, 0, c->stream>>>(lead->jobs, 1);
    if (int rc = check_launch(c, "k_trk_lk")) return rc;
    if (any_reject) {
        k_trk_reject<<<ns, kRejT, 0, c->stream>>>(lead->jobs);
        if (int rc = check_launch(c, "k_trk_reject")) return rc;
    }
    k_trk_update<<<ns, kTrkMaxPts, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_trk_update")) return rc;
    k_trk_response<<<dim3((unsigned)max_tiles, ns), kTrkT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_trk_response")) return rc;
    k_trk_nms<<<dim3(trk_blocks(max_np), ns), kTrkT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_trk_nms")) return rc;
    k_trk_select<<<ns, kTrkT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_trk_select")) return rc;
    k_trk_finish<<<ns, kTrkMaxPts, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_trk_finish")) return rc;
    HIP_TRY(c, hipMemcpyAsync(n_out, lead->counts, sizeof(int) * (size_t)n_streams, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int s = 0; s < n_streams; s++) {
        lmono_tracker *t = trks[s];
        t->frames++; t->prev_time = times[s];
        if (records_out && records_out[s] && n_out[s] > 0)
            HIP_TRY(c, hipMemcpyAsync(records_out[s], t->job.rec, sizeof(lmono_track_record) * (size_t)n_out[s], hipMemcpyDeviceToHost, c->stream));
        t->rej_ran = t->rej_on;
        if (t->rej_on) {
            HIP_TRY(c, hipMemcpyAsync(t->last_stats, t->rej_stats, sizeof(t->last_stats), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(t->last_F, t->rej_F, sizeof(t->last_F), hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int s = 0; s < n_streams; s++) { trks[s]->cur ^= 1; trks[s]->stale = false; }
    return LMONO_OK;
}

extern "C" int lmono_tracker_track(lmono_ctx *c, lmono_tracker *t, double time, const uint8_t *image_h, int format, lmono_track_record *records_out, int cap, int *n_out)
{
    if (!c || !t || t->ctx != c || !image_h || !n_out || (format != LMONO_TRACK_GREY8 && format != LMONO_TRACK_BGR8)) return LMONO_EINVAL;
    HIP_TRY(c, hipMemcpyAsync(t->image, image_h, (size_t)t->job.w * t->job.h * (format == LMONO_TRACK_BGR8 ? 3 : 1), hipMemcpyHostToDevice, c->stream));
    const uint8_t *img = t->image;
    return lmono_tracker_track_batch(c, 1, &t, &time, &img, format, &records_out, &cap, n_out);
}

extern "C" int lmono_tracker_pyramid(lmono_ctx *c, lmono_tracker *t, int level, uint8_t *image_h, int16_t *dx_h, int16_t *dy_h, int *width, int *height)
{
    if (!c || !t || t->ctx != c || level < 0) return LMONO_EINVAL;
    if (level >= t->job.n_levels) {
        if (width) *width = 0;
        if (height) *height = 0;
        return t->job.n_levels;
    }
    if (t->frames == 0 && (image_h || dx_h || dy_h)) { c->err = "lmono_tracker_pyramid: no frame tracked yet"; return LMONO_EINVAL; }
    const TrkLevel &L = t->pyr[t->cur].lv[level];
    const size_t np = (size_t)L.w * L.h;
    if (width) *width = L.w;
    if (height) *height = L.h;
    if (image_h) HIP_TRY(c, hipMemcpyAsync(image_h, L.img, np, hipMemcpyDeviceToHost, c->stream));
    if (dx_h) HIP_TRY(c, hipMemcpyAsync(dx_h, L.dx, np * sizeof(short), hipMemcpyDeviceToHost, c->stream));
    if (dy_h) HIP_TRY(c, hipMemcpyAsync(dy_h, L.dy, np * sizeof(short), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return t->job.n_levels;
}

extern "C" int lmono_tracker_response(lmono_ctx *c, lmono_tracker *t, float *response_h)
{
    if (!c || !t || t->ctx != c || !response_h) return LMONO_EINVAL;
    HIP_TRY(c, hipMemcpyAsync(response_h, t->job.resp, sizeof(float) * (size_t)t->job.w * t->job.h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return LMONO_OK;
}

extern "C" int lmono_tracker_lk(lmono_ctx *c, lmono_tracker *t, int n, const float *pts_h, float *fwd_h, float *rev_h, uint8_t *status_h)
{
    if (!c || !t || t->ctx != c || n < 0 || n > kTrkMaxPts || !pts_h || !fwd_h || !rev_h || !status_h) return LMONO_EINVAL;
    if (t->frames < 2) { c->err = "lmono_tracker_lk: needs two tracked frames"; return LMONO_EINVAL; }
    if (n == 0) return LMONO_OK;
    if (int rc = trk_job_table(c, t, 1, "lmono_tracker_lk")) return rc;
    TrkJob j = t->job;
    j.cur = t->pyr[t->cur]; j.prev = t->pyr[t->cur ^ 1];
    j.lk_n = n; j.lk_pts = t->lk_pts;
    HIP_TRY(c, hipMemcpyAsync(t->lk_pts, pts_h, sizeof(float2) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(t->jobs, &j, sizeof(TrkJob), hipMemcpyHostToDevice, c->stream));
    const unsigned lk_blocks = (unsigned)((n + kTrkT / kWave - 1) / (kTrkT / kWave));
    k_trk_lk<<<dim3(lk_blocks, 1), kTrkT, 0, c->stream>>>(t->jobs, 0);
    if (int rc = check_launch(c, "k_trk_lk")) return rc;
    k_trk_lk<<<dim3(lk_blocks, 1), kTrkT, 0, c->stream>>>(t->jobs, 1);
    if (int rc = check_launch(c, "k_trk_lk")) return rc;
    std::vector<unsigned char> sf((size_t)n), sb((size_t)n);
    HIP_TRY(c, hipMemcpyAsync(fwd_h, j.cur_pts, sizeof(float2) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(rev_h, j.rev_pts, sizeof(float2) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sf.data(), j.st_f, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sb.data(), j.st_b, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++) { status_h[2 * i] = sf[(size_t)i]; status_h[2 * i + 1] = sb[(size_t)i]; }
    return LMONO_OK;
}

extern "C" int lmono_tracker_reject_f(lmono_ctx *c, lmono_tracker *t, int n, const float *prev_px_h, const float *cur_px_h, uint32_t frame_key,
                                      uint8_t *status_h, int32_t *stats, double *F)
{
    if (!c || !t || t->ctx != c || !prev_px_h || !cur_px_h || !status_h) return LMONO_EINVAL;
    if (!t->rej_on) { c->err = "lmono_tracker_reject_f: rejection is off; call lmono_tracker_set_reject_f first"; return LMONO_EINVAL; }
    if (n < 8 || n > kTrkMaxPts) { c->err = "lmono_tracker_reject_f: n must be in 8..512"; return LMONO_EINVAL; }
    if (int rc = trk_job_table(c, t, 1, "lmono_tracker_reject_f")) return rc;
    TrkJob j = t->job;
    trk_reject_job(t, j, n, frame_key);
    HIP_TRY(c, hipMemcpyAsync(t->rej_prev, prev_px_h, sizeof(float2) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(t->rej_cur, cur_px_h, sizeof(float2) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(t->jobs, &j, sizeof(TrkJob), hipMemcpyHostToDevice, c->stream));
    k_trk_reject<<<1, kRejT, 0, c->stream>>>(t->jobs);
    if (int rc = check_launch(c, "k_trk_reject")) return rc;
    int32_t st[4]; double Fd[9];
    HIP_TRY(c, hipMemcpyAsync(status_h, t->rej_st, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(st, t->rej_stats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(Fd, t->rej_F, sizeof(Fd), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 4 && stats; k++) stats[k] = st[k];
    for (int k = 0; k < 9 && F; k++) F[k] = Fd[k];
    return LMONO_OK;
}
