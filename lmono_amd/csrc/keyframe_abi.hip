// keyframe_abi.hip -- C ABI of the keyframe descriptor store (included by lmono_hip.hip after lmono_ctx is defined)
#pragma once
#include "keyframe.hip"
#include "pnp.hip"
#include "bow.hip"

// a vocabulary tree on the device (bow_abi.hip): shared by its handle and by every store it is attached to, freed with the last of them
struct BowVocDev {
    lmono_ctx *ctx = nullptr;
    BowVoc v{};
    DevOwner mem;
};

struct lmono_keyframes {
    lmono_ctx *ctx = nullptr;
    int w = 0, h = 0, max_kf = 0, max_kp = 0, thr = 20, n_kf = 0;
    ColourCam cam{};
    bool have_frame = false;             // blur / score hold a frame
    unsigned char *image = nullptr;      // staging of the host-buffer entry ([h][w][3])
    unsigned char *blur = nullptr, *score = nullptr;
    int *row_cnt = nullptr, *row_off = nullptr;
    char4 *pat = nullptr;
    // the store, slot-major
    int *n_kp_d = nullptr;               // [max_kf]
    float2 *kp = nullptr, *norm = nullptr;               // [max_kf][max_kp]
    uint32_t *desc = nullptr;                            // [max_kf][max_kp][8]
    float2 *win_uv = nullptr;                            // [max_kf][512]
    uint32_t *win_desc = nullptr;                        // [max_kf][512][8]
    std::vector<int> n_kp_h, n_win_h;                    // per stored keyframe
    DevOwner mem;
    // job table + results of a batch led by this store
    KfJob *jobs = nullptr;
    int *res = nullptr;
    int jobs_cap = 0;
    // outputs of lmono_keyframes_match, grown to the largest n_old seen
    int match_cap = 0;
    int *old_slot = nullptr, *m_index = nullptr, *m_dist = nullptr, *m_counts = nullptr;
    unsigned int *m_keys = nullptr;
    unsigned char *m_status = nullptr;
    float2 *m_uv = nullptr, *m_norm = nullptr;
    // lmono_keyframes_verify (pnp_abi.hip): the current keyframe's 3-D points, and per candidate job, status, pose [7] and stats [4]
    int verify_cap = 0;
    float *v_p3 = nullptr;
    PnpJob *v_jobs = nullptr;
    std::vector<PnpJob> v_jobs_h;                        // the upload's source: outlives every early return
    unsigned char *v_status = nullptr;
    double *v_pose = nullptr;
    int *v_stats = nullptr;
    // the loop detector's database (bow_abi.hip): the attached vocabulary, and the BoW vectors of keyframes [0, bow_done)
    std::shared_ptr<BowVocDev> voc;
    int bow_done = 0;
    int *bow_word = nullptr, *bow_n = nullptr;           // [max_kf][max_kp], [max_kf]
    double *bow_val = nullptr;                           // [max_kf][max_kp]
    double *q_s = nullptr;                               // [max_kf] score sums and flags of a query of this store
    int *q_flag = nullptr;
    // job tables and results of a build / query batch led by this store
    BowWordsJob *b_wjobs = nullptr;
    BowVecJob *b_vjobs = nullptr;
    int b_cap = 0;
    BowQueryJob *q_jobs = nullptr;
    BowResult *q_out = nullptr;
    int q_cap = 0;
};

extern "C" void lmono_keyframes_destroy(lmono_keyframes *k) { delete k; }

extern "C" int lmono_keyframes_clear(lmono_ctx *c, lmono_keyframes *k)
{
    if (!c || !k || k->ctx != c) return LMONO_EINVAL;
    k->n_kf = 0; k->n_kp_h.clear(); k->n_win_h.clear();
    k->bow_done = 0;
    return LMONO_OK;
}

extern "C" int lmono_keyframes_size(lmono_ctx *c, lmono_keyframes *k) { return (!c || !k || k->ctx != c) ? LMONO_EINVAL : k->n_kf; }

extern "C" lmono_keyframes *lmono_keyframes_create(lmono_ctx *c, const lmono_camera *cam, const lmono_brief_pattern *pattern, int max_keyframes, int max_keypoints, int fast_threshold)
{
    if (!c) return nullptr;
    if (!cam || !pattern || cam->width < 16 || cam->height < 16 || cam->width > 8192 || cam->height > 8192 || !(cam->fx != 0.0) || !(cam->fy != 0.0) ||
        max_keyframes < 1 || max_keyframes > 65535 || max_keypoints < 1 || max_keypoints > 65535 || fast_threshold < 0 || fast_threshold > 254) {
        c->err = "lmono_keyframes_create: bad camera / limits (image sides 16..8192, 1 <= max_keyframes <= 65535, 1 <= max_keypoints <= 65535, 0 <= fast_threshold <= 254)";
        return nullptr;
    }
    char4 pat[256];
    for (int i = 0; i < 256; i++) {
        const int v[4] = { pattern->x1[i], pattern->y1[i], pattern->x2[i], pattern->y2[i] };
        for (int q = 0; q < 4; q++)
            if (v[q] < -63 || v[q] > 63) { c->err = "lmono_keyframes_create: a pattern offset lies outside -63..63"; return nullptr; }
        pat[i] = make_char4((signed char)v[0], (signed char)v[1], (signed char)v[2], (signed char)v[3]);
    }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return nullptr; }
    lmono_keyframes *k = new lmono_keyframes();
    k->ctx = c;
    k->w = cam->width; k->h = cam->height; k->max_kf = max_keyframes; k->max_kp = max_keypoints; k->thr = fast_threshold ? fast_threshold : 20;
    colour_cam_from(*cam, k->cam);
    DevOwner &m = k->mem;
    const size_t np = (size_t)k->w * k->h, slots = (size_t)max_keyframes, per = (size_t)max_keypoints;
    bool ok = m.alloc(k->image, np * 3) && m.alloc(k->blur, np) && m.alloc(k->score, np) && m.alloc(k->row_cnt, (size_t)k->h) && m.alloc(k->row_off, (size_t)k->h) &&
              m.alloc(k->pat, 256) && m.alloc(k->n_kp_d, slots) && m.alloc(k->kp, slots * per) && m.alloc(k->norm, slots * per) && m.alloc(k->desc, slots * per * 8) &&
              m.alloc(k->win_uv, slots * kKfMaxWin) && m.alloc(k->win_desc, slots * kKfMaxWin * 8);
    ok = ok && hipMemcpy(k->pat, pat, sizeof(pat), hipMemcpyHostToDevice) == hipSuccess && hipMemset(k->n_kp_d, 0, slots * sizeof(int)) == hipSuccess;
    if (!ok) { c->err = "lmono_keyframes_create: device allocation failed"; lmono_keyframes_destroy(k); return nullptr; }
    return k;
}

extern "C" int lmono_keyframes_add_batch(lmono_ctx *c, int n, lmono_keyframes *const *kfs, const uint8_t *const *image_d, int format, const int *n_window,
                                         const float *const *window_uv_h, int *index_out, int *n_keypoints_out)
{
    if (!c || n <= 0 || !kfs || !image_d || !n_window || !window_uv_h || (format != LMONO_TRACK_GREY8 && format != LMONO_TRACK_BGR8)) return LMONO_EINVAL;
    for (int s = 0; s < n; s++) {
        const int fault = batch_handle_fault(c, s, kfs);
        if (fault == kHandleForeign || !image_d[s] || n_window[s] < 0 || n_window[s] > kKfMaxWin || (n_window[s] > 0 && !window_uv_h[s])) {
            c->err = "lmono_keyframes_add_batch: bad stream arguments (0 <= n_window <= 512)"; return LMONO_EINVAL;
        }
        if (fault == kHandleRepeated) { c->err = "lmono_keyframes_add_batch: stores must be distinct"; return LMONO_EINVAL; }
        if (kfs[s]->n_kf >= kfs[s]->max_kf) { c->err = "lmono_keyframes_add: the store is full"; return LMONO_ECAPACITY; }
    }
    lmono_keyframes *lead = kfs[0];
    if (!job_table(lead->mem, lead->jobs, lead->res, lead->jobs_cap, n, 2)) { c->err = "lmono_keyframes_add_batch: job table allocation failed"; return LMONO_ENOMEM; }
    std::vector<KfJob> jobs((size_t)n);
    int max_tiles = 1, max_h = 1, max_pts = 1;
    for (int s = 0; s < n; s++) {
        lmono_keyframes *k = kfs[s];
        const size_t slot = (size_t)k->n_kf;
        KfJob &j = jobs[(size_t)s];
        j.w = k->w; j.h = k->h; j.format = format; j.thr = k->thr; j.max_kp = k->max_kp; j.n_win = n_window[s];
        j.cam = k->cam; j.src = image_d[s]; j.blur = k->blur; j.score = k->score; j.row_cnt = k->row_cnt; j.row_off = k->row_off;
        j.res = lead->res + 2 * s; j.n_kp = k->n_kp_d + slot;
        j.kp = k->kp + slot * k->max_kp; j.norm = k->norm + slot * k->max_kp; j.desc = k->desc + slot * k->max_kp * 8;
        j.win_uv = k->win_uv + slot * kKfMaxWin; j.win_desc = k->win_desc + slot * kKfMaxWin * 8; j.pat = k->pat;
        if (n_window[s] > 0)
            HIP_TRY(c, hipMemcpyAsync(k->win_uv + slot * kKfMaxWin, window_uv_h[s], sizeof(float2) * (size_t)n_window[s], hipMemcpyHostToDevice, c->stream));
        max_tiles = std::max(max_tiles, ((k->w + kKfTW - 1) / kKfTW) * ((k->h + kKfTH - 1) / kKfTH));
        max_h = std::max(max_h, k->h); max_pts = std::max(max_pts, k->max_kp + n_window[s]);
    }
    const unsigned ns = (unsigned)n, row_blocks = (unsigned)((max_h + kKfT / kWave - 1) / (kKfT / kWave));
    HIP_TRY(c, hipMemcpyAsync(lead->jobs, jobs.data(), sizeof(KfJob) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    k_kf_blur<<<dim3((unsigned)max_tiles, ns), kKfT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_kf_blur")) return rc;
    k_kf_fast_score<<<dim3((unsigned)max_tiles, ns), kKfT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_kf_fast_score")) return rc;
    k_kf_fast_nms_count<<<dim3(row_blocks, ns), kKfT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_kf_fast_nms_count")) return rc;
    k_kf_fast_nms_scan<<<ns, kKfT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_kf_fast_nms_scan")) return rc;
    k_kf_fast_nms_write<<<dim3(row_blocks, ns), kKfT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_kf_fast_nms_write")) return rc;
    const unsigned brief_blocks = (unsigned)std::min((max_pts + kKfT / kWave - 1) / (kKfT / kWave), 2048);
    k_kf_brief<<<dim3(brief_blocks, ns), kKfT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_kf_brief")) return rc;
    std::vector<int> res((size_t)n * 2);
    HIP_TRY(c, hipMemcpyAsync(res.data(), lead->res, sizeof(int) * res.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    bool over = false;
    for (int s = 0; s < n; s++) {
        kfs[s]->have_frame = true;
        if (n_keypoints_out) n_keypoints_out[s] = res[2 * (size_t)s];
        over = over || res[2 * (size_t)s + 1] != 0;
    }
    if (over) { c->err = "lmono_keyframes_add: an image has more FAST corners than max_keypoints; no store was changed"; return LMONO_ECAPACITY; }
    for (int s = 0; s < n; s++) {
        lmono_keyframes *k = kfs[s];
        k->n_kp_h.push_back(res[2 * (size_t)s]); k->n_win_h.push_back(n_window[s]);
        if (index_out) index_out[s] = k->n_kf;
        k->n_kf++;
    }
    return LMONO_OK;
}

extern "C" int lmono_keyframes_add(lmono_ctx *c, lmono_keyframes *k, const uint8_t *image_h, int format, int n_window, const float *window_uv_h, int *index_out, int *n_keypoints_out)
{
    if (!c || !k || k->ctx != c || !image_h || (format != LMONO_TRACK_GREY8 && format != LMONO_TRACK_BGR8)) return LMONO_EINVAL;
    // everything lmono_keyframes_add_batch would refuse is refused before the image copy is queued: an early return leaves nothing in flight
    if (n_window < 0 || n_window > kKfMaxWin || (n_window > 0 && !window_uv_h)) { c->err = "lmono_keyframes_add: bad window arguments (0 <= n_window <= 512)"; return LMONO_EINVAL; }
    if (k->n_kf >= k->max_kf) { c->err = "lmono_keyframes_add: the store is full"; return LMONO_ECAPACITY; }
    HIP_TRY(c, hipMemcpyAsync(k->image, image_h, (size_t)k->w * k->h * (format == LMONO_TRACK_BGR8 ? 3 : 1), hipMemcpyHostToDevice, c->stream));
    const uint8_t *img = k->image;
    return lmono_keyframes_add_batch(c, 1, &k, &img, format, &n_window, &window_uv_h, index_out, n_keypoints_out);
}

extern "C" int lmono_keyframes_load(lmono_ctx *c, lmono_keyframes *k, int n_keypoints, const float *keypoints_h, const float *norm_h, const uint32_t *descriptors_h,
                                    int n_window, const float *window_uv_h, const uint32_t *window_descriptors_h, int *index_out)
{
    if (!c || !k || k->ctx != c || n_keypoints < 0 || n_window < 0 || n_window > kKfMaxWin || (n_keypoints > 0 && (!keypoints_h || !norm_h || !descriptors_h)) ||
        (n_window > 0 && (!window_uv_h || !window_descriptors_h))) return LMONO_EINVAL;
    if (n_keypoints > k->max_kp) { c->err = "lmono_keyframes_load: more keypoints than max_keypoints"; return LMONO_ECAPACITY; }
    if (k->n_kf >= k->max_kf) { c->err = "lmono_keyframes_load: the store is full"; return LMONO_ECAPACITY; }
    const size_t slot = (size_t)k->n_kf, nk = (size_t)n_keypoints, nw = (size_t)n_window;
    if (nk) {
        HIP_TRY(c, hipMemcpyAsync(k->kp + slot * k->max_kp, keypoints_h, sizeof(float2) * nk, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(k->norm + slot * k->max_kp, norm_h, sizeof(float2) * nk, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(k->desc + slot * k->max_kp * 8, descriptors_h, 32 * nk, hipMemcpyHostToDevice, c->stream));
    }
    if (nw) {
        HIP_TRY(c, hipMemcpyAsync(k->win_uv + slot * kKfMaxWin, window_uv_h, sizeof(float2) * nw, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(k->win_desc + slot * kKfMaxWin * 8, window_descriptors_h, 32 * nw, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(k->n_kp_d + slot, &n_keypoints, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    k->n_kp_h.push_back(n_keypoints); k->n_win_h.push_back(n_window);
    if (index_out) *index_out = k->n_kf;
    k->n_kf++;
    return LMONO_OK;
}

// The search of lmono_keyframes_match queued on the stream, its results left in the store's m_* arrays (nothing is read back or waited
// for).  The arguments are the caller's to check; n_win of cur is > 0.  Shared with lmono_keyframes_verify (pnp_abi.hip)
static int kf_match_launch(lmono_ctx *c, lmono_keyframes *k, int cur, int n_old, const int32_t *old_indices, int max_kp)
{
    const int n_win = k->n_win_h[(size_t)cur];
    if (k->match_cap < n_old) {
        // eight arrays of one capacity (nothing reads them now: every call ends synchronised).  match_cap is 0 from a failed growth to the next call, which grows all eight again
        const int old = k->match_cap;
        int cap = 0;
        k->match_cap = 0;
        auto grow = [&](auto *&p, size_t per) { cap = old; return k->mem.grow_replace(p, cap, (size_t)n_old, /*floor=*/4, per); };
        if (!grow(k->old_slot, 1) || !grow(k->m_keys, kKfMaxWin) || !grow(k->m_status, kKfMaxWin) || !grow(k->m_index, kKfMaxWin) || !grow(k->m_dist, kKfMaxWin) ||
            !grow(k->m_uv, kKfMaxWin) || !grow(k->m_norm, kKfMaxWin) || !grow(k->m_counts, 1)) { c->err = "lmono_keyframes_match: device allocation failed"; return LMONO_ENOMEM; }
        k->match_cap = cap;
    }
    const size_t e = (size_t)n_old * n_win;
    KfMatchJob mj;
    mj.cur_desc = k->win_desc + (size_t)cur * kKfMaxWin * 8; mj.n_win = n_win; mj.n_old = n_old; mj.old_slot = k->old_slot; mj.n_kp = k->n_kp_d;
    mj.desc = k->desc; mj.kp = k->kp; mj.norm = k->norm; mj.max_kp = k->max_kp; mj.keys = k->m_keys; mj.status = k->m_status; mj.index = k->m_index; mj.dist = k->m_dist;
    mj.old_uv = k->m_uv; mj.old_norm = k->m_norm; mj.counts = k->m_counts;
    HIP_TRY(c, hipMemcpyAsync(k->old_slot, old_indices, sizeof(int) * (size_t)n_old, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)k->m_keys, (int)kKfNoMatch, e, c->stream));
    const unsigned shares = (unsigned)std::max(1, (max_kp + kKfShare - 1) / kKfShare);
    k_kf_match<<<dim3(shares, (unsigned)n_old), kKfT, 0, c->stream>>>(mj);
    if (int rc = check_launch(c, "k_kf_match")) return rc;
    k_kf_match_finish<<<(unsigned)n_old, kKfMaxWin, 0, c->stream>>>(mj);
    return check_launch(c, "k_kf_match_finish");
}

extern "C" int lmono_keyframes_match(lmono_ctx *c, lmono_keyframes *k, int cur, int n_old, const int32_t *old_indices, uint8_t *status_h, int32_t *index_h, int32_t *dist_h,
                                     float *old_uv_h, float *old_norm_h, int32_t *counts_h)
{
    if (!c || !k || k->ctx != c || cur < 0 || cur >= k->n_kf || n_old < 1 || n_old > 65535 || !old_indices) return LMONO_EINVAL;
    int max_kp = 0;
    for (int o = 0; o < n_old; o++) {
        if (old_indices[o] < 0 || old_indices[o] >= k->n_kf) { c->err = "lmono_keyframes_match: an old index is not a stored keyframe"; return LMONO_EINVAL; }
        max_kp = std::max(max_kp, k->n_kp_h[(size_t)old_indices[o]]);
    }
    const int n_win = k->n_win_h[(size_t)cur];
    if (n_win == 0) {
        for (int o = 0; o < n_old && counts_h; o++) counts_h[o] = 0;
        return LMONO_OK;
    }
    if (int rc = kf_match_launch(c, k, cur, n_old, old_indices, max_kp)) return rc;
    const size_t e = (size_t)n_old * n_win;
    if (status_h) HIP_TRY(c, hipMemcpyAsync(status_h, k->m_status, e, hipMemcpyDeviceToHost, c->stream));
    if (index_h) HIP_TRY(c, hipMemcpyAsync(index_h, k->m_index, sizeof(int) * e, hipMemcpyDeviceToHost, c->stream));
    if (dist_h) HIP_TRY(c, hipMemcpyAsync(dist_h, k->m_dist, sizeof(int) * e, hipMemcpyDeviceToHost, c->stream));
    if (old_uv_h) HIP_TRY(c, hipMemcpyAsync(old_uv_h, k->m_uv, sizeof(float2) * e, hipMemcpyDeviceToHost, c->stream));
    if (old_norm_h) HIP_TRY(c, hipMemcpyAsync(old_norm_h, k->m_norm, sizeof(float2) * e, hipMemcpyDeviceToHost, c->stream));
    if (counts_h) HIP_TRY(c, hipMemcpyAsync(counts_h, k->m_counts, sizeof(int) * (size_t)n_old, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return LMONO_OK;
}

extern "C" int lmono_keyframes_images(lmono_ctx *c, lmono_keyframes *k, uint8_t *blur_h, uint8_t *score_h)
{
    if (!c || !k || k->ctx != c) return LMONO_EINVAL;
    if (!k->have_frame) { c->err = "lmono_keyframes_images: no image added yet"; return LMONO_EINVAL; }
    const size_t np = (size_t)k->w * k->h;
    if (blur_h) HIP_TRY(c, hipMemcpyAsync(blur_h, k->blur, np, hipMemcpyDeviceToHost, c->stream));
    if (score_h) HIP_TRY(c, hipMemcpyAsync(score_h, k->score, np, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return LMONO_OK;
}

extern "C" int lmono_keyframes_get(lmono_ctx *c, lmono_keyframes *k, int index, int *n_keypoints, float *keypoints_h, float *norm_h, uint32_t *descriptors_h,
                                   int *n_window, float *window_uv_h, uint32_t *window_descriptors_h)
{
    if (!c || !k || k->ctx != c || index < 0 || index >= k->n_kf) return LMONO_EINVAL;
    const size_t slot = (size_t)index, nk = (size_t)k->n_kp_h[slot], nw = (size_t)k->n_win_h[slot];
    if (n_keypoints) *n_keypoints = (int)nk;
    if (n_window) *n_window = (int)nw;
    if (nk && keypoints_h) HIP_TRY(c, hipMemcpyAsync(keypoints_h, k->kp + slot * k->max_kp, sizeof(float2) * nk, hipMemcpyDeviceToHost, c->stream));
    if (nk && norm_h) HIP_TRY(c, hipMemcpyAsync(norm_h, k->norm + slot * k->max_kp, sizeof(float2) * nk, hipMemcpyDeviceToHost, c->stream));
    if (nk && descriptors_h) HIP_TRY(c, hipMemcpyAsync(descriptors_h, k->desc + slot * k->max_kp * 8, 32 * nk, hipMemcpyDeviceToHost, c->stream));
    if (nw && window_uv_h) HIP_TRY(c, hipMemcpyAsync(window_uv_h, k->win_uv + slot * kKfMaxWin, sizeof(float2) * nw, hipMemcpyDeviceToHost, c->stream));
    if (nw && window_descriptors_h) HIP_TRY(c, hipMemcpyAsync(window_descriptors_h, k->win_desc + slot * kKfMaxWin * 8, 32 * nw, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return LMONO_OK;
}
