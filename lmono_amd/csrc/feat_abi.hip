// feat_abi.hip -- C ABI of the per-feature kernels and the marginalisation: feat.hip, marg.hip (included by lmono_hip.hip after lmono_ctx is defined)
#pragma once
#include "feat_check.hpp"
// ---- per-feature kernels (triangulation, depth refinement, outlier scores, depth shift) ---------------------------
static int feat_setup(lmono_ctx *c, DevBuf &db, FeatBatch &B, int n_windows, const int *feat_off, const double *Rs, const double *Ps, const double *tlc,
                      const int *start_frame, const int *obs_off, const double *pts, const double *depth, int track_cnt, const char *refine_err = nullptr)
{
    if (!c || n_windows <= 0 || !feat_off || !Rs || !Ps || !tlc || !start_frame || !obs_off || !pts || !depth) return LMONO_EINVAL;
    // the descriptor's structure, on the host and before anything is uploaded or launched: the kernels index Rs / Ps / pts by it without a check of their own
    const char *bad = feat_check_tracks(n_windows, feat_off, start_frame, obs_off, track_cnt);
    if (!bad) bad = refine_err;
    if (bad) { c->err = std::string("per-feature kernels: ") + bad; return LMONO_EINVAL; }
    HIP_TRY(c, hipSetDevice(c->device));
    const int F = feat_off[n_windows];
    for (int w = 0; w < n_windows; w++) if (feat_off[w + 1] - feat_off[w] > LMONO_BA_MAX_FEATURES) { c->err = "more than LMONO_BA_MAX_FEATURES (" + std::to_string(LMONO_BA_MAX_FEATURES) + ") tracks in a window"; return LMONO_ECAPACITY; }
    const int TO = F > 0 ? obs_off[F] : 0;
    bool ok = true;
    B.n_windows = n_windows;
    B.feat_off = db.up(feat_off, (size_t)n_windows + 1, ok);
    B.Rs = db.up(Rs, (size_t)n_windows * 99, ok); B.Ps = db.up(Ps, (size_t)n_windows * 33, ok); B.tlc = db.up(tlc, (size_t)n_windows * 16, ok);
    B.start_frame = db.up(start_frame, (size_t)F, ok); B.obs_off = db.up(obs_off, (size_t)F + 1, ok); B.pts = db.up(pts, (size_t)TO * 2, ok);
    B.depth = db.up(depth, (size_t)F, ok);
    B.solve_flag = db.up((const int *)nullptr, (size_t)F, ok); B.score = db.up((const double *)nullptr, (size_t)F, ok);
    B.x = nullptr; B.cand = nullptr;
    db.ready(ok);
    if (!ok) { c->err = "per-feature kernels: device allocation / upload failed"; return LMONO_ENOMEM; }
    return LMONO_OK;
}

extern "C" int lmono_triangulate(lmono_ctx *c, int n_windows, const int *feat_off_h, const double *Rs_h, const double *Ps_h, const double *tlc_h,
                                 const int *start_frame_h, const int *obs_off_h, const double *pts_h, double *depth_h, int *solve_flag_h,
                                 int track_cnt, int window_size, double factor_weight, int refine_max_iter)
{
    DevBuf db(c); FeatBatch B{};
    int rc = feat_setup(c, db, B, n_windows, feat_off_h, Rs_h, Ps_h, tlc_h, start_frame_h, obs_off_h, pts_h, depth_h, track_cnt,
                        feat_check_refine(window_size, refine_max_iter, LMONO_FEAT_MAX_REFINE_ITER));
    if (rc) return rc;
    B.track_cnt = track_cnt; B.window_size = window_size; B.weight = factor_weight; B.max_iter = refine_max_iter;
    const int F = feat_off_h[n_windows];
    if (F == 0) return LMONO_OK;
    hipLaunchKernelGGL(k_triangulate_init, dim3((F + 127) / 128), dim3(128), 0, c->stream, B);
    if (refine_max_iter >= 0) {
        // one observation per thread when every window's (track, observation) pairs fit the kernel's LDS (the Estimator's windows do): a quarter of the time.
        // One big window sends the whole batch to the 256-thread kernel.  A window of up to 256 tracks gets the same bits from either kernel (a track per
        // thread in both, so the block sums group alike): tests/test_feat_gpu.py asserts equal bytes for a 200-track window across the 1024-track and the
        // 3072-observation limit.  Above 256 tracks a thread of the 256-thread kernel owns tracks tid, tid + 256, ..., so its block sums group differently
        // and equal bits are not guaranteed; what is asserted there is agreement of both kernels with the oracle at 1e-9 of the inverse depth.  Measured
        // on an MI355X: a 600-track window (4 observations each, 18 iterations) came out byte for byte the same from both kernels all the same -- the
        // sums feed only the accept / reject decisions and the radius, and a last-bit change of a radius >= 1e4 does not reach a step's bits.
        bool items = true;
        for (int w = 0; w < n_windows && items; w++) {
            const int nf = feat_off_h[w + 1] - feat_off_h[w];
            const int no = nf > 0 ? obs_off_h[feat_off_h[w + 1]] - obs_off_h[feat_off_h[w]] : 0;
            if (nf > kDrT || no > kDrItems) items = false;
        }
        if (items) hipLaunchKernelGGL(k_depth_refine_items, dim3(n_windows), dim3(kDrT), 0, c->stream, B);
        else hipLaunchKernelGGL(k_depth_refine, dim3(n_windows), dim3(256), 0, c->stream, B);
    }
    rc = check_launch(c, "k_triangulate_init/k_depth_refine");
    if (rc) return rc;
    bool ok = db.down(depth_h, B.depth, sizeof(double) * F);
    if (solve_flag_h && refine_max_iter >= 0) ok = ok && db.down(solve_flag_h, B.solve_flag, sizeof(int) * F);
    if (!ok || !db.fetch()) { c->err = "lmono_triangulate: read-back failed"; return LMONO_ENODEV; }      // the results are in the caller's arrays
    return LMONO_OK;
}

extern "C" int lmono_outlier_scores(lmono_ctx *c, int n_windows, const int *feat_off_h, const double *Rs_h, const double *Ps_h, const double *tlc_h,
                                    const int *start_frame_h, const int *obs_off_h, const double *pts_h, const double *depth_h,
                                    int track_cnt, double factor_weight, double *score_h)
{
    if (!score_h) return LMONO_EINVAL;
    DevBuf db(c); FeatBatch B{};
    int rc = feat_setup(c, db, B, n_windows, feat_off_h, Rs_h, Ps_h, tlc_h, start_frame_h, obs_off_h, pts_h, depth_h, track_cnt);
    if (rc) return rc;
    B.track_cnt = track_cnt; B.window_size = 0; B.weight = factor_weight; B.max_iter = 0;
    const int F = feat_off_h[n_windows];
    if (F == 0) return LMONO_OK;
    hipLaunchKernelGGL(k_outlier_scores, dim3((F + 127) / 128), dim3(128), 0, c->stream, B);
    rc = check_launch(c, "k_outlier_scores");
    if (rc) return rc;
    if (!db.down(score_h, B.score, sizeof(double) * F) || !db.fetch()) { c->err = "lmono_outlier_scores: read-back failed"; return LMONO_ENODEV; }
    return LMONO_OK;
}

extern "C" int lmono_shift_depth(lmono_ctx *c, const double *back_R0, const double *back_P0, const double *R1, const double *P1, const double *tlc,
                                 int n, const double *pt_i_h, const double *depth_h, double *depth_out_h)
{
    if (!c || !back_R0 || !back_P0 || !R1 || !P1 || !tlc || n < 0 || !pt_i_h || !depth_h || !depth_out_h) return LMONO_EINVAL;
    if (n == 0) return LMONO_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    double poses[40];
    memcpy(poses, back_R0, 72); memcpy(poses + 9, back_P0, 24); memcpy(poses + 12, R1, 72); memcpy(poses + 21, P1, 24); memcpy(poses + 24, tlc, 128);
    DevBuf db(c); bool ok = true;
    double *pd = db.up(poses, 40, ok), *pt = db.up(pt_i_h, (size_t)n * 2, ok), *d = db.up(depth_h, (size_t)n, ok), *o = db.up((const double *)nullptr, (size_t)n, ok);
    db.ready(ok);
    if (!ok) { c->err = "lmono_shift_depth: device allocation / upload failed"; return LMONO_ENOMEM; }
    hipLaunchKernelGGL(k_shift_depth, dim3((n + 127) / 128), dim3(128), 0, c->stream, (const double *)pd, n, (const double *)pt, (const double *)d, o, (const int *)nullptr);
    int rc = check_launch(c, "k_shift_depth");
    if (rc) return rc;
    if (!db.down(depth_out_h, o, sizeof(double) * n) || !db.fetch()) { c->err = "lmono_shift_depth: read-back failed"; return LMONO_ENODEV; }
    return LMONO_OK;
}

extern "C" int lmono_shift_depth_batch(lmono_ctx *c, int n_windows, const double *frames_h, const int *track_off_h,
                                       const double *pt_i_h, const double *depth_h, double *depth_out_h)
{
    if (!c || n_windows <= 0 || !frames_h || !track_off_h) return LMONO_EINVAL;
    if (const char *bad = feat_check_offsets(n_windows, track_off_h)) { c->err = std::string("lmono_shift_depth_batch: ") + bad; return LMONO_EINVAL; }
    const int n = track_off_h[n_windows];
    if (n == 0) return LMONO_OK;
    if (!pt_i_h || !depth_h || !depth_out_h) return LMONO_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<int> win((size_t)n);
    for (int w = 0; w < n_windows; w++) {
        for (int f = track_off_h[w]; f < track_off_h[w + 1]; f++) win[(size_t)f] = w;
    }
    DevBuf db(c); bool ok = true;
    double *pd = db.up(frames_h, (size_t)n_windows * 40, ok), *pt = db.up(pt_i_h, (size_t)n * 2, ok), *d = db.up(depth_h, (size_t)n, ok);
    int *wd = db.up(win.data(), (size_t)n, ok);
    double *o = db.up((const double *)nullptr, (size_t)n, ok);
    db.ready(ok);
    if (!ok) { c->err = "lmono_shift_depth_batch: device allocation / upload failed"; return LMONO_ENOMEM; }
    hipLaunchKernelGGL(k_shift_depth, dim3((n + 127) / 128), dim3(128), 0, c->stream, (const double *)pd, n, (const double *)pt, (const double *)d, o, (const int *)wd);
    int rc = check_launch(c, "k_shift_depth");
    if (rc) return rc;
    if (!db.down(depth_out_h, o, sizeof(double) * n) || !db.fetch()) { c->err = "lmono_shift_depth_batch: read-back failed"; return LMONO_ENODEV; }
    return LMONO_OK;
}

// ---- marginalisation prior ----------------------------------------------------------------------------------------
extern "C" int lmono_marginalize(lmono_ctx *c, int n_windows, const int *feat_off_h, const int *obs_off_h, const double *poses_h, const double *ex_h,
                                 const double *inv_depth_h, const int *obs_feat_h, const int *obs_j_h, const double *obs_pts_h,
                                 const double *laser01_h, const double *laser_info_h, const double *mono_info_h,
                                 double *lin_J_h, double *lin_r_h, int *status_h)
{
    if (!c || n_windows <= 0 || !feat_off_h || !obs_off_h || !poses_h || !ex_h || !laser01_h || !laser_info_h || !mono_info_h || !lin_J_h || !lin_r_h) return LMONO_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    const char *bad = feat_check_offsets(n_windows, feat_off_h);
    if (!bad) bad = feat_check_offsets(n_windows, obs_off_h);
    if (bad) { c->err = std::string("lmono_marginalize: ") + bad; return LMONO_EINVAL; }
    const int TF = feat_off_h[n_windows], TO = obs_off_h[n_windows];
    // an array that the counts say is not empty must be there: up() takes a null source for scratch that nothing has to fill, and the kernel would read it
    if ((TF > 0 && !inv_depth_h) || (TO > 0 && (!obs_feat_h || !obs_j_h || !obs_pts_h))) {
        c->err = "lmono_marginalize: inv_depth / obs_feat / obs_j / obs_pts must not be null when there are tracks / observations"; return LMONO_EINVAL;
    }
    std::vector<int> fo((size_t)TF + 1, 0);
    for (int w = 0; w < n_windows; w++) {
        if (feat_off_h[w + 1] - feat_off_h[w] > kMargMaxF0) { c->err = "lmono_marginalize: more than 160 tracks anchored at frame 0"; return LMONO_ECAPACITY; }
        int o = obs_off_h[w];
        for (int f = feat_off_h[w]; f < feat_off_h[w + 1]; f++) {
            fo[f] = o;
            unsigned seen = 0;      // frames of this track so far: the kernel keeps ONE W_d row per (track, frame) and assigns it
            while (o < obs_off_h[w + 1] && obs_feat_h[o] == f - feat_off_h[w]) {
                if (obs_j_h[o] < 1 || obs_j_h[o] > 10) { c->err = "lmono_marginalize: observation frame must be 1..10"; return LMONO_EINVAL; }
                if (seen & (1u << obs_j_h[o])) { c->err = "lmono_marginalize: a track is observed twice in the same frame"; return LMONO_EINVAL; }
                seen |= 1u << obs_j_h[o];
                o++;
            }
        }
        if (o != obs_off_h[w + 1]) { c->err = "lmono_marginalize: observations are not grouped by track"; return LMONO_EINVAL; }
    }
    fo[TF] = TO;
    double info[40];
    memcpy(info, laser_info_h, 36 * sizeof(double)); memcpy(info + 36, mono_info_h, 4 * sizeof(double));
    DevBuf db(c); bool ok = true;
    MargBatch B{};
    B.n_windows = n_windows;
    B.feat_off = db.up(feat_off_h, (size_t)n_windows + 1, ok); B.obs_off = db.up(obs_off_h, (size_t)n_windows + 1, ok);
    B.poses = db.up(poses_h, (size_t)n_windows * 77, ok); B.ex = db.up(ex_h, (size_t)n_windows * 7, ok);
    B.inv_depth = db.up(inv_depth_h, (size_t)TF, ok); B.feat_obs_off = db.up(fo.data(), (size_t)TF + 1, ok);
    B.obs_j = db.up(obs_j_h, (size_t)TO, ok); B.obs_pts = db.up(obs_pts_h, (size_t)TO * 4, ok);
    B.laser01 = db.up(laser01_h, (size_t)n_windows * 24, ok); B.info = db.up(info, (size_t)40, ok);
    B.lin_J = db.up((const double *)nullptr, (size_t)n_windows * kMargN * kMargN, ok); B.lin_r = db.up((const double *)nullptr, (size_t)n_windows * kMargN, ok);
    B.status = db.up((const int *)nullptr, (size_t)n_windows, ok);
    db.ready(ok);
    if (!ok) { c->err = "lmono_marginalize: device allocation / upload failed"; return LMONO_ENOMEM; }
    hipLaunchKernelGGL(k_marginalize, dim3(n_windows), dim3(kMgT), sizeof(MargLds), c->stream, B);
    int rc = check_launch(c, "k_marginalize");
    if (rc) return rc;
    // (the three outputs are neighbours in the scratch: one copy through the pinned staging buffer)
    bool got = db.down(lin_J_h, B.lin_J, sizeof(double) * (size_t)n_windows * kMargN * kMargN) && db.down(lin_r_h, B.lin_r, sizeof(double) * (size_t)n_windows * kMargN);
    if (got && status_h) got = db.down(status_h, B.status, sizeof(int) * (size_t)n_windows);
    if (!got || !db.fetch()) { c->err = "lmono_marginalize: read-back failed"; return LMONO_ENODEV; }      // the results are in the caller's arrays
    return LMONO_OK;
}

extern "C" int lmono_marg_evaluate(lmono_ctx *c, int n_windows, const double *lin_J_h, const double *lin_r_h, const double *x0_h, const double *x_h, double *residual_h)
{
    if (!c || n_windows <= 0 || !lin_J_h || !lin_r_h || !x0_h || !x_h || !residual_h) return LMONO_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf db(c); bool ok = true;
    const double *J = db.up(lin_J_h, (size_t)n_windows * kMargN * kMargN, ok), *r = db.up(lin_r_h, (size_t)n_windows * kMargN, ok);
    const double *x0 = db.up(x0_h, (size_t)n_windows * 77, ok), *x = db.up(x_h, (size_t)n_windows * 77, ok);
    double *res = db.up((const double *)nullptr, (size_t)n_windows * kMargN, ok);
    db.ready(ok);
    if (!ok) { c->err = "lmono_marg_evaluate: device allocation / upload failed"; return LMONO_ENOMEM; }
    hipLaunchKernelGGL(k_marg_evaluate, dim3(n_windows), dim3(128), 0, c->stream, n_windows, J, r, x0, x, res);
    int rc = check_launch(c, "k_marg_evaluate");
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(residual_h, res, sizeof(double) * (size_t)n_windows * kMargN, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // the results are in the caller's arrays
    return LMONO_OK;
}


// MARGIN_SECOND_NEW (Estimator.cc:1406-1470): the previous prior loses one of its blocks.
extern "C" int lmono_marg_second_new(lmono_ctx *c, int n_windows, int n_blocks, int drop_block, const double *lin_J_h, const double *lin_r_h,
                                     const double *x0_h, const double *x_h, double *lin_J_out_h, double *lin_r_out_h, int *status_h)
{
    if (!c || n_windows <= 0 || n_blocks < 2 || n_blocks > 11 || drop_block < 0 || drop_block >= n_blocks || !lin_J_h || !lin_r_h || !x0_h || !x_h ||
        !lin_J_out_h || !lin_r_out_h) return LMONO_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n0 = 6 * (size_t)n_blocks, n = n0 - 6, W = (size_t)n_windows;
    DevBuf db(c); bool ok = true;
    Marg2Batch B{};
    B.n_windows = n_windows; B.nb = n_blocks; B.drop = drop_block;
    B.lin_J = db.up(lin_J_h, W * n0 * n0, ok); B.lin_r = db.up(lin_r_h, W * n0, ok);
    B.x0 = db.up(x0_h, W * n_blocks * 7, ok); B.x = db.up(x_h, W * n_blocks * 7, ok);
    B.out_J = db.up((const double *)nullptr, W * n * n, ok); B.out_r = db.up((const double *)nullptr, W * n, ok);
    B.status = db.up((const int *)nullptr, W, ok);
    db.ready(ok);
    if (!ok) { c->err = "lmono_marg_second_new: device allocation / upload failed"; return LMONO_ENOMEM; }
    hipLaunchKernelGGL(k_marg_second_new, dim3(n_windows), dim3(kMgT), sizeof(Marg2Lds), c->stream, B);
    int rc = check_launch(c, "k_marg_second_new");
    if (rc) return rc;
    bool got = db.down(lin_J_out_h, B.out_J, sizeof(double) * W * n * n) && db.down(lin_r_out_h, B.out_r, sizeof(double) * W * n);
    if (got && status_h) got = db.down(status_h, B.status, sizeof(int) * W);
    if (!got || !db.fetch()) { c->err = "lmono_marg_second_new: read-back failed"; return LMONO_ENODEV; }      // the results are in the caller's arrays
    return LMONO_OK;
}
