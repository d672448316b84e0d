// oracle/cpu_shim.cpp -- TEST INFRASTRUCTURE, not a backend of the product.
//
// The Estimator-path subset of the C ABI (include/lmono_hip.h) implemented on the CPU oracle's C functions (oracle/lo_*.c), so that the
// C++ host mirror (lmono_amd/host/lmono_host.cpp: Estimator::processImage and everything under it) can be linked against the ORACLE instead
// of liblmono_hip.so.  The result is oracle/estimator_seq_cpu: the reference's frame loop in C++ over the restated Ceres / Eigen numerics, one
// thread -- the CPU baseline of `bench.py --workload ba-seq` (VERDICT r3 #2 v: the Python replay oracle/estimator_ref.py pays interpreter
// time per frame), and a second check of estimator_ref.py (tests/test_estimator_loop_cpu.py: the two print the same trajectory).
// Only tests/ and bench.py's cpu_baseline leg build or run it; nothing under lmono_amd/ links it, and the product still fails without a GPU.
// PARITY UNPINNED like the rest of oracle/ (DESIGN.md section 2).
#include "../include/lmono_hip.h"
#include "../lmono_amd/csrc/feat_check.hpp"      // the descriptor checks of the per-track entry points: the HIP library's own, plain C++

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

extern "C" {
typedef struct {
    int n_poses, n_feat, n_obs;
    int use_prior, ex_constant, use_mono, max_iter;
    double *poses, *ex, *inv_depth;
    const int32_t *obs_feat, *obs_i, *obs_j;
    const double *obs_pts, *laser_consts, *laser_info, *mono_info, *prior_T, *prior_w;
} lo_ba_problem;                              // oracle/lo_ba_solve.c
typedef struct { double initial_cost, final_cost; int iterations, termination, n_successful, n_unsuccessful; } lo_ba_summary;
int lo_ba_solve(lo_ba_problem *p, lo_ba_summary *sum);
void lo_triangulate_init(const double *Rs, const double *Ps, const double *tlc, int n_feat, const int32_t *start_frame, const int32_t *obs_off,
                         const double *pts, double *depth, int track_cnt);
void lo_depth_refine(const double *Rs, const double *Ps, const double *tlc, int n_feat, const int32_t *start_frame, const int32_t *obs_off,
                     const double *pts, double *depth, int32_t *solve_flag, int track_cnt, int window_size, double weight, int max_iter);
void lo_outlier_scores(const double *Rs, const double *Ps, const double *tlc, int n_feat, const int32_t *start_frame, const int32_t *obs_off,
                       const double *pts, const double *depth, int track_cnt, double weight, double *score);
void lo_shift_depth(const double *back_R0, const double *back_P0, const double *R1s, const double *P1s, const double *tlc, int n,
                    const double *pt_i, const double *depth, double *depth_out);
int lo_marginalize(const double *poses, const double *ex, int n_f0, const double *inv_depth, int n_obs, const int32_t *obs_feat,
                   const int32_t *obs_j, const double *obs_pts, const double *laser_consts01, const double *laser_info, const double *mono_info,
                   double *lin_J, double *lin_r, int *m_out);
int lo_marg_second_new(int nb, int drop, const double *lin_J, const double *lin_r, const double *x0, const double *x, double *out_J, double *out_r);
}

struct lmono_ctx { std::string err; };
struct lmono_ba_batch {
    int W = 0, max_iter = 30;
    std::vector<int> feat_off, obs_off, flags, obs_feat, obs_i, obs_j;
    std::vector<double> poses, ex, invd, obs_pts, laser, prior_T, laser_info, mono_info, prior_w, summary;
};

extern "C" {

lmono_ctx *lmono_create(int) { return new lmono_ctx(); }
void lmono_destroy(lmono_ctx *c) { delete c; }
const char *lmono_last_error(const lmono_ctx *c) { return c ? c->err.c_str() : "null context"; }
int lmono_use_own_stream(lmono_ctx *c) { return c ? LMONO_OK : LMONO_EINVAL; }

static int ba_load(lmono_ctx *c, lmono_ba_batch *b, const lmono_ba_desc *d)
{
    if (!d || d->n_windows <= 0) { c->err = "cpu shim: bad descriptor"; return LMONO_EINVAL; }
    const int W = d->n_windows, TF = d->feat_off[W], TO = d->obs_off[W];
    b->W = W;
    b->feat_off.assign(d->feat_off, d->feat_off + W + 1); b->obs_off.assign(d->obs_off, d->obs_off + W + 1);
    b->flags.assign(d->flags, d->flags + 4 * W);
    b->poses.assign(d->poses, d->poses + (size_t)W * 77); b->ex.assign(d->ex, d->ex + (size_t)W * 7);
    b->invd.assign(TF > 0 ? d->inv_depth : nullptr, TF > 0 ? d->inv_depth + TF : nullptr);
    if (TO > 0) {
        b->obs_feat.assign(d->obs_feat, d->obs_feat + TO); b->obs_i.assign(d->obs_i, d->obs_i + TO); b->obs_j.assign(d->obs_j, d->obs_j + TO);
        b->obs_pts.assign(d->obs_pts, d->obs_pts + (size_t)TO * 4);
    } else { b->obs_feat.clear(); b->obs_i.clear(); b->obs_j.clear(); b->obs_pts.clear(); }
    b->laser.assign(d->laser_consts, d->laser_consts + (size_t)W * 240); b->prior_T.assign(d->prior_T, d->prior_T + (size_t)W * 16);
    b->laser_info.assign(d->laser_info, d->laser_info + 36); b->mono_info.assign(d->mono_info, d->mono_info + 4); b->prior_w.assign(d->prior_w, d->prior_w + 2);
    b->summary.assign((size_t)W * 6, 0.0);
    return LMONO_OK;
}
lmono_ba_batch *lmono_ba_batch_create(lmono_ctx *c, const lmono_ba_desc *d)
{
    lmono_ba_batch *b = new lmono_ba_batch();
    if (ba_load(c, b, d) != LMONO_OK) { delete b; return nullptr; }
    return b;
}
void lmono_ba_batch_destroy(lmono_ba_batch *b) { delete b; }
int lmono_ba_batch_update(lmono_ctx *c, lmono_ba_batch *b, const lmono_ba_desc *d) { return ba_load(c, b, d); }
int lmono_ba_solve(lmono_ctx *, lmono_ba_batch *b, int max_iterations)
{
    for (int w = 0; w < b->W; w++) {
        lo_ba_problem p;
        const int f0 = b->feat_off[w], o0 = b->obs_off[w];
        p.n_poses = b->flags[4 * w]; p.n_feat = b->feat_off[w + 1] - f0; p.n_obs = b->obs_off[w + 1] - o0;
        p.use_prior = b->flags[4 * w + 1]; p.ex_constant = b->flags[4 * w + 2]; p.use_mono = b->flags[4 * w + 3]; p.max_iter = max_iterations;
        static double dzero = 0.0; static int32_t izero = 0;
        p.poses = b->poses.data() + (size_t)w * 77; p.ex = b->ex.data() + (size_t)w * 7; p.inv_depth = p.n_feat ? b->invd.data() + f0 : &dzero;
        p.obs_feat = p.n_obs ? b->obs_feat.data() + o0 : &izero; p.obs_i = p.n_obs ? b->obs_i.data() + o0 : &izero; p.obs_j = p.n_obs ? b->obs_j.data() + o0 : &izero;
        p.obs_pts = p.n_obs ? b->obs_pts.data() + (size_t)o0 * 4 : &dzero;
        p.laser_consts = b->laser.data() + (size_t)w * 240; p.laser_info = b->laser_info.data(); p.mono_info = b->mono_info.data();
        p.prior_T = b->prior_T.data() + (size_t)w * 16; p.prior_w = b->prior_w.data();
        lo_ba_summary sm;
        lo_ba_solve(&p, &sm);
        double *s = b->summary.data() + (size_t)w * 6;
        s[0] = sm.initial_cost; s[1] = sm.final_cost; s[2] = sm.iterations; s[3] = sm.termination; s[4] = sm.n_successful; s[5] = sm.n_unsuccessful;
    }
    return LMONO_OK;
}
int lmono_ba_batch_read(lmono_ctx *, lmono_ba_batch *b, double *poses_h, double *ex_h, double *inv_depth_h, double *summary_h)
{
    if (poses_h) std::memcpy(poses_h, b->poses.data(), sizeof(double) * b->poses.size());
    if (ex_h) std::memcpy(ex_h, b->ex.data(), sizeof(double) * b->ex.size());
    if (inv_depth_h && !b->invd.empty()) std::memcpy(inv_depth_h, b->invd.data(), sizeof(double) * b->invd.size());
    if (summary_h) std::memcpy(summary_h, b->summary.data(), sizeof(double) * b->summary.size());
    return LMONO_OK;
}

// the per-track entry points refuse what liblmono_hip.so refuses (feat_abi.hip: feat_setup), before they touch an output array
static int feat_refuse(lmono_ctx *c, const char *bad)
{
    if (c) c->err = std::string("per-feature kernels: ") + bad;
    return LMONO_EINVAL;
}

int lmono_triangulate(lmono_ctx *c, int n_windows, const int *feat_off_h, const double *Rs_h, const double *Ps_h, const double *tlc_h,
                      const int *start_frame_h, const int *obs_off_h, const double *pts_h, double *depth_h, int *solve_flag_h,
                      int track_cnt, int window_size, double factor_weight, int refine_max_iter)
{
    if (!c || n_windows <= 0 || !feat_off_h || !Rs_h || !Ps_h || !tlc_h || !start_frame_h || !obs_off_h || !pts_h || !depth_h) return LMONO_EINVAL;
    const char *bad = lmono::feat_check_tracks(n_windows, feat_off_h, start_frame_h, obs_off_h, track_cnt);
    if (!bad) bad = lmono::feat_check_refine(window_size, refine_max_iter, LMONO_FEAT_MAX_REFINE_ITER);
    if (bad) return feat_refuse(c, bad);
    for (int w = 0; w < n_windows; w++) {
        const int f0 = feat_off_h[w], nf = feat_off_h[w + 1] - f0;
        if (nf <= 0) continue;
        lo_triangulate_init(Rs_h + (size_t)w * 99, Ps_h + (size_t)w * 33, tlc_h + (size_t)w * 16, nf, start_frame_h + f0, obs_off_h + f0, pts_h, depth_h + f0, track_cnt);
        if (refine_max_iter >= 0) {
            std::vector<int32_t> flag((size_t)nf, 0);
            lo_depth_refine(Rs_h + (size_t)w * 99, Ps_h + (size_t)w * 33, tlc_h + (size_t)w * 16, nf, start_frame_h + f0, obs_off_h + f0, pts_h, depth_h + f0,
                            flag.data(), track_cnt, window_size, factor_weight, refine_max_iter);
            if (solve_flag_h) for (int f = 0; f < nf; f++) solve_flag_h[f0 + f] = flag[(size_t)f];
        }
    }
    return LMONO_OK;
}
int lmono_outlier_scores(lmono_ctx *c, int n_windows, const int *feat_off_h, const double *Rs_h, const double *Ps_h, const double *tlc_h,
                         const int *start_frame_h, const int *obs_off_h, const double *pts_h, const double *depth_h,
                         int track_cnt, double factor_weight, double *score_h)
{
    if (!c || !score_h || n_windows <= 0 || !feat_off_h || !Rs_h || !Ps_h || !tlc_h || !start_frame_h || !obs_off_h || !pts_h || !depth_h) return LMONO_EINVAL;
    if (const char *bad = lmono::feat_check_tracks(n_windows, feat_off_h, start_frame_h, obs_off_h, track_cnt)) return feat_refuse(c, bad);
    for (int w = 0; w < n_windows; w++) {
        const int f0 = feat_off_h[w], nf = feat_off_h[w + 1] - f0;
        if (nf > 0) lo_outlier_scores(Rs_h + (size_t)w * 99, Ps_h + (size_t)w * 33, tlc_h + (size_t)w * 16, nf, start_frame_h + f0, obs_off_h + f0, pts_h, depth_h + f0,
                                      track_cnt, factor_weight, score_h + f0);
    }
    return LMONO_OK;
}
int lmono_shift_depth(lmono_ctx *c, const double *back_R0, const double *back_P0, const double *R1, const double *P1, const double *tlc,
                      int n, const double *pt_i_h, const double *depth_h, double *depth_out_h)
{
    if (!c || !back_R0 || !back_P0 || !R1 || !P1 || !tlc || n < 0 || !pt_i_h || !depth_h || !depth_out_h) return LMONO_EINVAL;
    if (n > 0) lo_shift_depth(back_R0, back_P0, R1, P1, tlc, n, pt_i_h, depth_h, depth_out_h);
    return LMONO_OK;
}
int lmono_shift_depth_batch(lmono_ctx *c, int n_windows, const double *frames_h, const int *track_off_h, const double *pt_i_h, const double *depth_h, double *depth_out_h)
{
    if (!c || n_windows <= 0 || !frames_h || !track_off_h) return LMONO_EINVAL;
    if (const char *bad = lmono::feat_check_offsets(n_windows, track_off_h)) { c->err = std::string("lmono_shift_depth_batch: ") + bad; return LMONO_EINVAL; }
    if (track_off_h[n_windows] > 0 && (!pt_i_h || !depth_h || !depth_out_h)) return LMONO_EINVAL;
    for (int w = 0; w < n_windows; w++) {
        const int f0 = track_off_h[w], n = track_off_h[w + 1] - f0;
        const double *fr = frames_h + (size_t)w * 40;
        if (n > 0) lo_shift_depth(fr, fr + 9, fr + 12, fr + 21, fr + 24, n, pt_i_h + (size_t)f0 * 2, depth_h + f0, depth_out_h + f0);
    }
    return LMONO_OK;
}
int lmono_marginalize(lmono_ctx *, int n_windows, const int *feat_off_h, const int *obs_off_h, const double *poses_h, const double *ex_h,
                      const double *inv_depth_h, const int *obs_feat_h, const int *obs_j_h, const double *obs_pts_h,
                      const double *laser01_h, const double *laser_info_h, const double *mono_info_h,
                      double *lin_J_h, double *lin_r_h, int *status_h)
{
    for (int w = 0; w < n_windows; w++) {
        const int f0 = feat_off_h[w], nf = feat_off_h[w + 1] - f0, o0 = obs_off_h[w], no = obs_off_h[w + 1] - o0;
        // the ABI's observation -> track index is window-local already
        int m = 0;
        const int rc = lo_marginalize(poses_h + (size_t)w * 77, ex_h + (size_t)w * 7, nf, inv_depth_h + f0, no, obs_feat_h + o0, obs_j_h + o0, obs_pts_h + (size_t)o0 * 4,
                                      laser01_h + (size_t)w * 24, laser_info_h, mono_info_h, lin_J_h + (size_t)w * 66 * 66, lin_r_h + (size_t)w * 66, &m);
        if (status_h) status_h[w] = 0;
        if (rc != 0) return LMONO_EINVAL;
    }
    return LMONO_OK;
}
int lmono_marg_second_new(lmono_ctx *, int n_windows, int n_blocks, int drop_block, const double *lin_J_h, const double *lin_r_h,
                          const double *x0_h, const double *x_h, double *lin_J_out_h, double *lin_r_out_h, int *status_h)
{
    const int n0 = 6 * n_blocks, n = n0 - 6;
    for (int w = 0; w < n_windows; w++) {
        const int rc = lo_marg_second_new(n_blocks, drop_block, lin_J_h + (size_t)w * n0 * n0, lin_r_h + (size_t)w * n0, x0_h + (size_t)w * n_blocks * 7,
                                          x_h + (size_t)w * n_blocks * 7, lin_J_out_h + (size_t)w * n * n, lin_r_out_h + (size_t)w * n);
        if (status_h) status_h[w] = 0;
        if (rc != 0) return LMONO_EINVAL;
    }
    return LMONO_OK;
}

} // extern "C"
