// pnp_abi.hip -- C ABI of the loop verification: lmono_pnp_ransac, the PnP step on given problems, and
// lmono_keyframes_verify, findConnection from searchByBRIEFDes to the published loop (included by lmono_hip.hip behind keyframe_abi.hip)
#pragma once
#include "pnp.hip"

namespace {

struct PnpPrm { double thr; int n_hyp; unsigned int seed; int min_brief, min_pnp; double angle, trans; };

// the defaults of kitti_loop_config_04.yaml where a field is 0; false (c->err set) for a value outside its range
bool pnp_params(lmono_ctx *c, const lmono_pnp_params *p, const char *who, PnpPrm &o)
{
    static const lmono_pnp_params zero = { 0.0, 0, 0u, 0, 0, 0.0, 0.0 };
    if (!p) p = &zero;
    if (const char *bad = pnp_check_params(p->threshold, p->n_hyp, p->min_brief_loop_num, p->min_pnp_loop_num, p->angle_threshold, p->trans_threshold)) {
        c->err = std::string(who) + ": " + bad; return false;
    }
    o.thr = p->threshold != 0.0 ? p->threshold : 10.0 / 460.0;
    o.n_hyp = p->n_hyp ? p->n_hyp : 256;
    o.seed = p->seed;
    o.min_brief = p->min_brief_loop_num ? p->min_brief_loop_num : 25;
    o.min_pnp = p->min_pnp_loop_num ? p->min_pnp_loop_num : 5;
    o.angle = p->angle_threshold != 0.0 ? p->angle_threshold : 30.0;
    o.trans = p->trans_threshold != 0.0 ? p->trans_threshold : 20.0;
    return true;
}

bool pnp_pose_ok(const double *tq)
{
    for (int e = 0; e < 7; e++) if (!std::isfinite(tq[e])) return false;
    const double n = tq[3] * tq[3] + tq[4] * tq[4] + tq[5] * tq[5] + tq[6] * tq[6];
    return n > 0.25 && n < 4.0;          // a quaternion, if not an exactly normalised one
}

} // namespace

extern "C" int lmono_pnp_ransac(lmono_ctx *c, const lmono_pnp_params *params, int n, const int32_t *counts_h, const float *points_3d_h, const float *points_2d_h,
                                const double *guess_tq_h, const uint32_t *keys_h, uint8_t *status_h, double *pose_tq_h, int32_t *stats_h)
{
    if (!c || n < 1 || n > 65535 || !counts_h || !guess_tq_h || !keys_h) return LMONO_EINVAL;
    PnpPrm prm;
    if (!pnp_params(c, params, "lmono_pnp_ransac", prm)) return LMONO_EINVAL;
    size_t total = 0;
    for (int s = 0; s < n; s++) {
        if (counts_h[s] < 0) { c->err = "lmono_pnp_ransac: a count is negative"; return LMONO_EINVAL; }
        if (counts_h[s] > kPnpPts) { c->err = "lmono_pnp_ransac: a problem has more than 512 pairs"; return LMONO_ECAPACITY; }
        if (!pnp_pose_ok(guess_tq_h + 7 * (size_t)s)) { c->err = "lmono_pnp_ransac: a guess is not finite or its quaternion is far from unit length"; return LMONO_EINVAL; }
        total += (size_t)counts_h[s];
    }
    if (total > 0 && (!points_3d_h || !points_2d_h || !status_h)) return LMONO_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf buf(c);
    bool ok = true;
    const float *p3 = buf.up(points_3d_h, total * 3, ok), *p2 = buf.up(points_2d_h, total * 2, ok);
    unsigned char *st = buf.up((const unsigned char *)nullptr, total, ok);
    double *pose = buf.up((const double *)nullptr, (size_t)n * 7, ok);
    int *stats = buf.up((const int *)nullptr, (size_t)n * 4, ok);
    if (!ok) { c->err = "lmono_pnp_ransac: device allocation failed"; return LMONO_ENOMEM; }
    std::vector<PnpJob> jobs((size_t)n);
    size_t at = 0;
    for (int s = 0; s < n; s++) {
        PnpJob &j = jobs[(size_t)s];
        j.p3 = p3 + 3 * at; j.p2 = p2 + 2 * at; j.sel = nullptr; j.count = nullptr; j.n_src = counts_h[s]; j.gate = 0; j.n_hyp = prm.n_hyp;
        j.seed = prm.seed; j.key = keys_h[s]; j.thr2 = prm.thr * prm.thr;
        for (int e = 0; e < 7; e++) j.guess[e] = guess_tq_h[7 * (size_t)s + e];
        j.status = st + at; j.pose = pose + 7 * (size_t)s; j.stats = stats + 4 * (size_t)s;
        at += (size_t)counts_h[s];
    }
    const PnpJob *jobs_d = buf.up(jobs.data(), jobs.size(), ok);
    buf.ready(ok);
    if (!ok) { c->err = "lmono_pnp_ransac: upload failed"; return LMONO_ENOMEM; }
    k_pnp_ransac<<<(unsigned)n, kPnpT, 0, c->stream>>>(jobs_d);
    if (int rc = check_launch(c, "k_pnp_ransac")) return rc;
    if (total) HIP_TRY(c, hipMemcpyAsync(status_h, st, total, hipMemcpyDeviceToHost, c->stream));
    if (pose_tq_h) HIP_TRY(c, hipMemcpyAsync(pose_tq_h, pose, sizeof(double) * 7 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (stats_h) HIP_TRY(c, hipMemcpyAsync(stats_h, stats, sizeof(int) * 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return LMONO_OK;
}

extern "C" int lmono_keyframes_verify(lmono_ctx *c, lmono_keyframes *k, int cur, int n_old, const int32_t *old_indices, const float *point_3d_h, const double *vio_tq,
                                      const double *ex_tq, const double *old_tq_h, const lmono_pnp_params *params, int32_t *brief_counts_h, int32_t *pnp_inliers_h,
                                      uint8_t *status_h, double *pnp_tq_old_h, double *loop_info_h, uint8_t *has_loop_h, double *channel_h, double *relative_euler_h,
                                      double *pose_tq_h, int32_t *stats_h)
{
    if (!c || !k || k->ctx != c || cur < 0 || cur >= k->n_kf || n_old < 1 || n_old > 65535 || !old_indices || !vio_tq || !ex_tq) return LMONO_EINVAL;
    PnpPrm prm;
    if (!pnp_params(c, params, "lmono_keyframes_verify", prm)) return LMONO_EINVAL;
    if (!pnp_pose_ok(vio_tq) || !pnp_pose_ok(ex_tq)) { c->err = "lmono_keyframes_verify: vio_tq / ex_tq is not finite or its quaternion is far from unit length"; return LMONO_EINVAL; }
    if (channel_h && !old_tq_h) { c->err = "lmono_keyframes_verify: the 15-value channel needs old_tq_h"; return LMONO_EINVAL; }
    int max_kp = 0;
    for (int o = 0; o < n_old; o++) {
        if (old_indices[o] < 0 || old_indices[o] >= k->n_kf) { c->err = "lmono_keyframes_verify: an old index is not a stored keyframe"; return LMONO_EINVAL; }
        if (old_tq_h && !pnp_pose_ok(old_tq_h + 7 * (size_t)o)) { c->err = "lmono_keyframes_verify: an old pose is not finite or its quaternion is far from unit length"; return LMONO_EINVAL; }
        max_kp = std::max(max_kp, k->n_kp_h[(size_t)old_indices[o]]);
    }
    const int n_win = k->n_win_h[(size_t)cur];
    if (n_win > 0 && !point_3d_h) return LMONO_EINVAL;
    PnpPose G;
    pnp_guess(vio_tq, ex_tq, G);
    const double guess[7] = { G.t[0], G.t[1], G.t[2], G.q[0], G.q[1], G.q[2], G.q[3] };
    std::vector<int> counts((size_t)n_old, 0), stats((size_t)n_old * 4, -1);
    std::vector<double> pose((size_t)n_old * 7);
    for (int o = 0; o < n_old; o++) for (int e = 0; e < 7; e++) pose[7 * (size_t)o + e] = guess[e];
    if (n_win > 0) {
        HIP_TRY(c, hipSetDevice(c->device));
        if (k->verify_cap < n_old) {
            // four arrays of one capacity, grown like the eight of the match (every call ends synchronised)
            const int old = k->verify_cap;
            int cap = 0;
            k->verify_cap = 0;
            auto grow = [&](auto *&p, size_t per) { cap = old; return k->mem.grow_replace(p, cap, (size_t)n_old, /*floor=*/4, per); };
            if ((!k->v_p3 && !k->mem.alloc(k->v_p3, (size_t)kKfMaxWin * 3)) || !grow(k->v_jobs, 1) || !grow(k->v_status, kKfMaxWin) || !grow(k->v_pose, 7) || !grow(k->v_stats, 4)) {
                c->err = "lmono_keyframes_verify: device allocation failed"; return LMONO_ENOMEM;
            }
            k->verify_cap = cap;
        }
        if (int rc = kf_match_launch(c, k, cur, n_old, old_indices, max_kp)) return rc;
        std::vector<PnpJob> &jobs = k->v_jobs_h;        // kept by the store: an early return below leaves the queued copy a live source
        jobs.resize((size_t)n_old);
        for (int o = 0; o < n_old; o++) {
            PnpJob &j = jobs[(size_t)o];
            j.p3 = k->v_p3; j.p2 = (const float *)(k->m_norm + (size_t)o * n_win); j.sel = k->m_status + (size_t)o * n_win; j.count = k->m_counts + o;
            j.n_src = n_win; j.gate = prm.min_brief; j.n_hyp = prm.n_hyp; j.seed = prm.seed; j.key = ((unsigned int)cur << 16) | (unsigned int)old_indices[o];
            j.thr2 = prm.thr * prm.thr;
            for (int e = 0; e < 7; e++) j.guess[e] = guess[e];
            j.status = k->v_status + (size_t)o * kKfMaxWin; j.pose = k->v_pose + 7 * (size_t)o; j.stats = k->v_stats + 4 * (size_t)o;
        }
        HIP_TRY(c, hipMemcpyAsync(k->v_p3, point_3d_h, sizeof(float) * 3 * (size_t)n_win, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(k->v_jobs, jobs.data(), sizeof(PnpJob) * (size_t)n_old, hipMemcpyHostToDevice, c->stream));
        k_pnp_ransac<<<(unsigned)n_old, kPnpT, 0, c->stream>>>(k->v_jobs);
        if (int rc = check_launch(c, "k_pnp_ransac")) return rc;
        HIP_TRY(c, hipMemcpyAsync(counts.data(), k->m_counts, sizeof(int) * (size_t)n_old, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(stats.data(), k->v_stats, sizeof(int) * 4 * (size_t)n_old, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(pose.data(), k->v_pose, sizeof(double) * 7 * (size_t)n_old, hipMemcpyDeviceToHost, c->stream));
        if (status_h) HIP_TRY(c, hipMemcpy2DAsync(status_h, (size_t)n_win, k->v_status, (size_t)kKfMaxWin, (size_t)n_win, (size_t)n_old, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    for (int o = 0; o < n_old; o++) {
        const int *st = &stats[4 * (size_t)o];
        const int inliers = (st[0] > 0 && st[2] >= 4) ? st[2] : 0;
        PnpLoop L;
        pnp_after(&pose[7 * (size_t)o], vio_tq, ex_tq, prm.angle, prm.trans, L);
        const bool has_loop = counts[(size_t)o] > prm.min_brief && inliers > prm.min_pnp && L.within;
        if (brief_counts_h) brief_counts_h[o] = counts[(size_t)o];
        if (pnp_inliers_h) pnp_inliers_h[o] = inliers;
        if (has_loop_h) has_loop_h[o] = has_loop ? 1 : 0;
        if (pnp_tq_old_h) { double *d = pnp_tq_old_h + 7 * (size_t)o; for (int e = 0; e < 3; e++) d[e] = L.t_old[e]; for (int e = 0; e < 4; e++) d[3 + e] = L.q_old[e]; }
        if (loop_info_h) pnp_loop_info(L, loop_info_h + 8 * (size_t)o);
        if (relative_euler_h) for (int e = 0; e < 3; e++) relative_euler_h[3 * (size_t)o + e] = L.rel_euler[e];
        if (pose_tq_h) for (int e = 0; e < 7; e++) pose_tq_h[7 * (size_t)o + e] = pose[7 * (size_t)o + e];
        if (stats_h) for (int e = 0; e < 4; e++) stats_h[4 * (size_t)o + e] = st[e];
        if (channel_h) pnp_channel(old_tq_h + 7 * (size_t)o, L, cur, channel_h + 15 * (size_t)o);
    }
    return LMONO_OK;
}
