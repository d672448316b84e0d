// lidar_abi.hip -- C ABI of the LiDAR front end and odometry: frontend.hip, odometry.hip, corr_flat.hip (included by lmono_hip.hip after lmono_ctx is defined)
#pragma once
constexpr int kListGrid = 256;       // workgroups of k_correspond_list (fixed: the work list's length is only known on the device; almost always empty)

struct lmono_scan_batch {
    lmono_ctx *ctx = nullptr;
    int n_cap = 0;
    int64_t pts_cap = 0;
    int n_scans = 0;
    int64_t total = 0;
    int max_pts = 0;
    bool registered = false;
    bool grid_built = false;       // k_grid_build has run for this registration
    std::vector<int64_t> off_h;
    bool validation_pending = false;   // lmono_odom_shard_main_d ran: lmono_odom_shard_validate is the batch's first (whole) validation
    DevOwner mem;
    BatchView v{};
    int64_t *off_d = nullptr;
    float *in_owned = nullptr;     // staging buffer of lmono_scanreg_batch_h (pts_cap points), allocated on first use
    hipEvent_t staged_ev = nullptr, in_free_ev = nullptr;   // lmono_batch_stage_h: copy finished / the front end has read the staging buffer
    int64_t staged_points = -1;
    std::vector<int> feat_h;       // host copy of feat_n [n_scans][4], fetched on first use after a registration
    float *curv = nullptr;         // lmono_batch_get_curvature's curvature of the one scan asked for (k_curvature on demand)
    size_t curv_cap = 0;
    // odometry workspace
    int chains_cap = 0;
    double *state = nullptr, *incr = nullptr, *poses = nullptr, *xq = nullptr;
    int *corr = nullptr, *lm_info = nullptr, *corr_pair = nullptr, *seed = nullptr;
    float4 *crec = nullptr, *crec_pair = nullptr;
    float4 *lmrec = nullptr;               // the planes of k_lm_solve's staged blocks that are not in LDS: [chains_cap][4 - lm_planes][kMaxQueries]
    size_t lmrec_cap = 0;                  // float4 entries of lmrec
    unsigned int *wl = nullptr;            // work list of feature points the LDS tile search defers: [0] = count
    size_t wl_cap = 0;
    // boundary validation of the chained schedule
    double *ws = nullptr, *resid_d = nullptr;
    int *rstat = nullptr;
    unsigned int *rcount = nullptr;
    hipEvent_t rep_ev[2] = { nullptr, nullptr };
    lmono_boundary_report brep{};
    std::vector<double> resid_h;
    std::vector<int> rerun_h;
    int last_chains = 0, last_lead = 0, last_first = 0;
};

extern "C" void lmono_batch_destroy(lmono_scan_batch *b)
{
    if (!b) return;
    b->mem.clear();
    for (auto &e : b->rep_ev) if (e) (void)hipEventDestroy(e);
    if (b->staged_ev) (void)hipEventDestroy(b->staged_ev);
    if (b->in_free_ev) (void)hipEventDestroy(b->in_free_ev);
    delete b;
}

extern "C" lmono_scan_batch *lmono_batch_create(lmono_ctx *c, int n_cap, int64_t pts_cap)
{
    if (!c || n_cap <= 0 || pts_cap <= 0) return nullptr;
    if (hipSetDevice(c->device) != hipSuccess) return nullptr;
    lmono_scan_batch *b = new lmono_scan_batch();
    b->ctx = c; b->n_cap = n_cap; b->pts_cap = pts_cap;
    BatchView &v = b->v;
    const size_t T = (size_t)pts_cap, N = (size_t)n_cap;
    DevOwner &m = b->mem;
    bool ok = true;
    ok = ok && m.alloc(b->off_d, N + 1);
    ok = ok && m.alloc(v.cloud, T) && m.alloc(v.label, T);
    ok = ok && m.alloc(v.ring_tmp, T);
    ok = ok && m.alloc(v.seg_hist, ((T >> 10) + N + 1) * 64) && m.alloc(v.scan_ends, N * 2) && m.alloc(v.scan_half, N) && m.alloc(v.scan_ori, N * 4);
    ok = ok && m.alloc(v.ring_begin, N * 65) && m.alloc(v.n_cloud, N) && m.alloc(v.status, N);
    ok = ok && m.alloc(v.sel_sharp, N * 64 * 6 * 20) && m.alloc(v.sel_sharp_n, N * 64 * 6);
    ok = ok && m.alloc(v.sel_flat, N * 64 * 6 * 4) && m.alloc(v.sel_flat_n, N * 64 * 6);
    ok = ok && m.alloc(v.lf_tmp, T) && m.alloc(v.lf_n, N * 64) && m.alloc(v.vox_todo, N * 64 + 1) && m.alloc(v.sel_todo, N * 64 + 1) && m.alloc(v.li_todo, N * 2 + 1);
    ok = ok && m.alloc(v.sharp, N * kMaxSharp) && m.alloc(v.less_sharp, N * kMaxLessSharp);
    ok = ok && m.alloc(v.flat, N * kMaxFlat) && m.alloc(v.less_flat, T);
    ok = ok && m.alloc(v.feat_n, N * 4) && m.alloc(v.line_first_ge, N * 2 * 66) && m.alloc(v.line_last_le, N * 2 * 66);
    ok = ok && m.alloc(v.cg_cell, N * kCornerTable) && m.alloc(v.sg_cell, N * kSurfTable);
    ok = ok && m.alloc(v.cg_pts, N * kMaxLessSharp) && m.alloc(v.sg_pts, T) && m.alloc(v.grid_mask, N * 2);
    ok = ok && m.alloc(v.lbc_pts, N * kMaxLessSharp + kLbPad) && m.alloc(v.lbs_pts, T + kLbPad) && m.alloc(v.lb_start, N * 2 * (kLineKeys + 1)) && m.alloc(v.lb_elev, N * 2 * 66);
    ok = ok && m.alloc(b->incr, N * 7) && m.alloc(b->poses, N * 7) && m.alloc(b->xq, 8);
    ok = ok && m.alloc(b->corr_pair, (size_t)kMaxQueries * 4) && m.alloc(b->crec_pair, (size_t)kMaxQueries * 4);
    if (!ok) {
        c->err = "lmono_batch_create: hipMalloc failed";
        lmono_batch_destroy(b);
        return nullptr;
    }
    v.off = b->off_d;
    return b;
}

// rings a sensor can produce (scanRegistration keeps rings 0..50 of a 64-line sensor): grids of the per-ring kernels
static int rings_used(int n_lines) { return n_lines == 64 ? 51 : n_lines; }

// The front end (scanRegistration) over scans scan0 .. scan0 + n_scans - 1 of the batch: the per-scan kernels' grids cover n_scans scans, the
// batch view tells them where they start.  A whole-batch registration is (0, n); the online stream registers one slot at a time.
static int scanreg_launch(lmono_ctx *c, lmono_scan_batch *b, int scan0, int n_scans, int64_t max_pts, int n_limit = 0)
{
    BatchView v = b->v;
    v.scan0 = scan0; v.n_limit = n_limit;
    hipStream_t st = c->stream;
    c->ev = c->next_set();
    if (!c->ev) { c->err = "hipEventCreate failed"; return LMONO_ENODEV; }
    c->sets[c->n_sets - 1].reg = true;
    HIP_TRY(c, hipMemsetAsync(v.status + scan0, 0, sizeof(int) * n_scans, st));
    HIP_TRY(c, hipMemsetAsync(v.vox_todo, 0, sizeof(int), st));
    HIP_TRY(c, hipMemsetAsync(v.sel_todo, 0, sizeof(int), st));
    HIP_TRY(c, hipMemsetAsync(v.li_todo, 0, sizeof(int), st));
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    const int rt_tiles = (int)((max_pts + kRtTile - 1) / kRtTile);
    hipLaunchKernelGGL(k_ring_ends, dim3(n_scans), dim3(256), 0, st, v);
    if (rt_tiles > 0) hipLaunchKernelGGL(k_ring_tag, dim3(rt_tiles, n_scans), dim3(kRtT), 0, st, v);
    hipLaunchKernelGGL(k_ring_offsets, dim3(n_scans), dim3(64), 0, st, v);
    if (rt_tiles > 0) hipLaunchKernelGGL(k_ring_scatter, dim3(rt_tiles, n_scans), dim3(kRtT), 0, st, v);
    HIP_TRY(c, hipEventRecord(c->ev[1], st));
    // (nothing between these two: k_select computes the curvature itself; the slot keeps the layout of lmono_timing_read)
    HIP_TRY(c, hipEventRecord(c->ev[2], st));
    // the kernels below run one workgroup per ring of the sensor; the counters of the rings it cannot produce stay zero
    const int n_rings = rings_used(b->v.n_lines);
    HIP_TRY(c, hipMemsetAsync(v.sel_sharp_n + (size_t)scan0 * 64 * 6, 0, sizeof(int) * (size_t)n_scans * 64 * 6, st));
    HIP_TRY(c, hipMemsetAsync(v.sel_flat_n + (size_t)scan0 * 64 * 6, 0, sizeof(int) * (size_t)n_scans * 64 * 6, st));
    HIP_TRY(c, hipMemsetAsync(v.lf_n + (size_t)scan0 * 64, 0, sizeof(int) * (size_t)n_scans * 64, st));
    hipLaunchKernelGGL(k_select, dim3((n_rings + 3) / 4, n_scans), dim3(256), 4 * sel_slice_bytes(kSelSmallCap) + 4 * kSelScratch, st, v, kSelSmallCap, 0);
    hipLaunchKernelGGL(k_select, dim3(kSelBigGrid), dim3(256), 4 * sel_slice_bytes(kRingCap) + 4 * kSelScratch, st, v, (int)kRingCap, 1);
    HIP_TRY(c, hipEventRecord(c->ev[3], st));
    hipLaunchKernelGGL((k_voxel<kVoxSmallSlots, kVoxSmallBits, true>), dim3(n_rings, n_scans), dim3(256), kVoxLdsSmall, st, v);
    hipLaunchKernelGGL((k_voxel<kVoxBigSlots, kVoxBigBits, false>), dim3(kVoxBigGrid), dim3(256), kVoxLdsBig, st, v);
    HIP_TRY(c, hipEventRecord(c->ev[4], st));
    hipLaunchKernelGGL(k_compact_index, dim3(n_scans), dim3(kLiT), kLiLdsHalf, st, v);       // compaction + (line, bin) index of the two "last" clouds
    HIP_TRY(c, hipEventRecord(c->ev[5], st));
    // the hash grids serve the 32-lane-group search (LMONO_OPT_CORR_TILE 0) and the deferred lists of modes 1 and 2; the default
    // (flattened sweeps) works on the line index alone, so the grids are built on demand (ensure_grid)
#ifdef LMONO_DIAG_SEARCH
    if (c->opt[LMONO_OPT_CORR_TILE] != 3) {
        hipLaunchKernelGGL(k_grid_build, dim3(n_scans, 1 + kGridPar), dim3(1024), kGridLds, st, v);
        b->grid_built = true; v.has_grid = 1; b->v.has_grid = 1;
    }
#endif
    HIP_TRY(c, hipEventRecord(c->ev[6], st));
    hipLaunchKernelGGL(k_line_index<false>, dim3(kLiBigGrid), dim3(kLiT), kLiLdsFull, st, v);
    HIP_TRY(c, hipEventRecord(c->ev[7], st));
    return check_launch(c, "scanreg kernels");
}

extern "C" int lmono_scanreg_batch(lmono_ctx *c, lmono_scan_batch *b, const float *xyzi_d, const int64_t *offsets_h,
                                   int n_scans, int n_lines, float min_range);

// the batch's own input buffer (pts_cap points of xyzi), allocated by the first call that stages host points
static int batch_own_input(lmono_ctx *c, lmono_scan_batch *b)
{
    if (b->in_owned || b->mem.alloc(b->in_owned, (size_t)b->pts_cap * 4)) return LMONO_OK;
    const hipError_t e = hipGetLastError();
    c->err = std::string("hipMalloc(&q, (size_t)(b->pts_cap > 0 ? b->pts_cap : 1) * 16): ") + hipGetErrorString(e);      // the words this failure has always had
    return e == hipErrorOutOfMemory ? LMONO_ENOMEM : LMONO_ENODEV;
}

extern "C" int lmono_scanreg_batch_h(lmono_ctx *c, lmono_scan_batch *b, const float *xyzi_h, const int64_t *offsets_h,
                                     int n_scans, int n_lines, float min_range)
{
    if (!c || !b || !xyzi_h || !offsets_h || n_scans <= 0) return LMONO_EINVAL;
    if (offsets_h[0] != 0) { c->err = "offsets must start at 0"; return LMONO_EINVAL; }
    const int64_t total = offsets_h[n_scans];
    if (total < 0 || total > b->pts_cap) { c->err = "batch: too many points"; return LMONO_ECAPACITY; }
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = batch_own_input(c, b)) return rc;
    if (total > 0) {
        // staged: the caller's (pageable) buffer is free again when this returns
        HIP_TRY(c, hipMemcpyAsync(b->in_owned, xyzi_h, (size_t)total * 16, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return lmono_scanreg_batch(c, b, b->in_owned, offsets_h, n_scans, n_lines, min_range);
}

extern "C" int lmono_scanreg_batch(lmono_ctx *c, lmono_scan_batch *b, const float *xyzi_d, const int64_t *offsets_h,
                                   int n_scans, int n_lines, float min_range)
{
    if (!c || !b || !xyzi_d || !offsets_h || n_scans <= 0) return LMONO_EINVAL;
    if (n_lines != 16 && n_lines != 32 && n_lines != 64) { c->err = "n_lines must be 16, 32 or 64"; return LMONO_EINVAL; }
    if (n_scans > b->n_cap) { c->err = "batch: too many scans"; return LMONO_ECAPACITY; }
    int64_t max_pts = 0;
    for (int s = 0; s < n_scans; s++) {
        const int64_t m = offsets_h[s + 1] - offsets_h[s];
        if (m < 0 || m > INT_MAX / 2) { c->err = "bad offsets"; return LMONO_EINVAL; }
        max_pts = m > max_pts ? m : max_pts;
    }
    const int64_t total = offsets_h[n_scans] - offsets_h[0];
    if (offsets_h[0] != 0) { c->err = "offsets must start at 0"; return LMONO_EINVAL; }
    if (total > b->pts_cap) { c->err = "batch: too many points"; return LMONO_ECAPACITY; }
    HIP_TRY(c, hipSetDevice(c->device));
    b->off_h.assign(offsets_h, offsets_h + n_scans + 1);
    b->n_scans = n_scans; b->total = total; b->max_pts = (int)max_pts; b->registered = false; b->grid_built = false;
    b->feat_h.clear();
    BatchView &v = b->v;
    v.in = (const float4 *)xyzi_d; v.n_scans = n_scans; v.scan0 = 0; v.n_lines = n_lines; v.min_range = min_range; v.has_grid = 0;
    HIP_TRY(c, hipMemcpyAsync(b->off_d, b->off_h.data(), sizeof(int64_t) * (n_scans + 1), hipMemcpyHostToDevice, c->stream));
    int rc = scanreg_launch(c, b, 0, n_scans, max_pts);
    if (rc) return rc;
    b->registered = true;
    return LMONO_OK;
}

// ---- streamed input: H2D of the next working set beside the compute of the current one ---------------------------------------------
extern "C" int lmono_batch_stage_h(lmono_ctx *c, lmono_scan_batch *b, const float *xyzi_h, int64_t total_points)
{
    if (!c || !b || !xyzi_h || total_points < 0) return LMONO_EINVAL;
    if (total_points > b->pts_cap) { c->err = "batch: too many points"; return LMONO_ECAPACITY; }
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->copy_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    if (int rc = batch_own_input(c, b)) return rc;
    if (!b->staged_ev) HIP_TRY(c, hipEventCreateWithFlags(&b->staged_ev, hipEventDisableTiming));
    if (!b->in_free_ev) HIP_TRY(c, hipEventCreateWithFlags(&b->in_free_ev, hipEventDisableTiming));
    // the front end of this batch's previous registration may still read the staging buffer
    else HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, b->in_free_ev, 0));
    if (total_points > 0) HIP_TRY(c, hipMemcpyAsync(b->in_owned, xyzi_h, (size_t)total_points * 16, hipMemcpyHostToDevice, c->copy_stream));
    HIP_TRY(c, hipEventRecord(b->staged_ev, c->copy_stream));
    b->staged_points = total_points;
    return LMONO_OK;
}

extern "C" int lmono_scanreg_batch_staged(lmono_ctx *c, lmono_scan_batch *b, const int64_t *offsets_h, int n_scans, int n_lines, float min_range)
{
    if (!c || !b || !offsets_h || n_scans <= 0) return LMONO_EINVAL;
    if (b->staged_points < 0 || !b->in_owned) { c->err = "lmono_scanreg_batch_staged: nothing staged (lmono_batch_stage_h first)"; return LMONO_EINVAL; }
    if (offsets_h[n_scans] != b->staged_points) { c->err = "lmono_scanreg_batch_staged: offsets do not match the staged points"; return LMONO_EINVAL; }
    HIP_TRY(c, hipStreamWaitEvent(c->stream, b->staged_ev, 0));          // the device waits for the copy, the host does not
    const int rc = lmono_scanreg_batch(c, b, b->in_owned, offsets_h, n_scans, n_lines, min_range);
    HIP_TRY(c, hipEventRecord(b->in_free_ev, c->stream));
    b->staged_points = -1;
    return rc;
}

extern "C" int lmono_timing_reset(lmono_ctx *c)
{
    if (!c) return LMONO_EINVAL;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemset(c->stats_d, 0, 320));
    c->n_sets = 0;
    return LMONO_OK;
}

extern "C" int lmono_timing_read(lmono_ctx *c, double *ms, int cap, int *n_scanreg_calls, int *n_odom_calls)
{
    if (!c || !ms) return LMONO_EINVAL;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double sum[13] = { 0 };
    int nr = 0, no = 0;
    float t;
    for (int i = 0; i < c->n_sets; i++) {
        const EvSet &s = c->sets[i];
        if (s.reg) {
            nr++;
            if (hipEventElapsedTime(&t, s.e[0], s.e[7]) == hipSuccess) sum[0] += t;
            for (int k = 0; k < 7; k++)
                if (hipEventElapsedTime(&t, s.e[k], s.e[k + 1]) == hipSuccess) sum[2 + k] += t;
        }
        if (s.odom) {
            no++;
            if (hipEventElapsedTime(&t, s.e[8], s.e[9]) == hipSuccess) sum[1] += t;
            for (int k = 0; k + 2 < s.n_kev; k += 3) {
                if (k + 2 >= (int)s.kev.size()) break;
                if (hipEventElapsedTime(&t, s.kev[k], s.kev[k + 1]) == hipSuccess) sum[9] += t;
                if (hipEventElapsedTime(&t, s.kev[k + 1], s.kev[k + 2]) == hipSuccess) sum[10] += t;
                sum[11] += 1.0;
            }
        }
    }
    {
        unsigned long long st[40] = { 0 };
        HIP_TRY(c, hipMemcpy(st, c->stats_d, 320, hipMemcpyDeviceToHost));
        sum[12] = (double)st[0];
        for (int i = 1; i < 40 && 12 + i < cap; i++) ms[12 + i] = (double)st[i];     // diagnostic words (LMONO_TILE_PROF builds)
    }
    for (int i = 0; i < cap && i < 13; i++) ms[i] = sum[i];
    if (n_scanreg_calls) *n_scanreg_calls = nr;
    if (n_odom_calls) *n_odom_calls = no;
    return LMONO_OK;
}

extern "C" int lmono_batch_counts(lmono_ctx *c, lmono_scan_batch *b, int32_t *counts_h)
{
    if (!c || !b || !counts_h || !b->registered) return LMONO_EINVAL;
    const int n = b->n_scans;
    std::vector<int> nc(n), fn(n * 4), stt(n);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(nc.data(), b->v.n_cloud, sizeof(int) * n, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(fn.data(), b->v.feat_n, sizeof(int) * n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(stt.data(), b->v.status, sizeof(int) * n, hipMemcpyDeviceToHost));
    for (int s = 0; s < n; s++) {
        counts_h[6 * s] = nc[s];
        for (int k = 0; k < 4; k++) counts_h[6 * s + 1 + k] = fn[4 * s + k];
        counts_h[6 * s + 5] = stt[s];
    }
    return LMONO_OK;
}

extern "C" int lmono_batch_get_cloud(lmono_ctx *c, lmono_scan_batch *b, int scan, int which, float *out_h, int cap)
{
    if (!c || !b || !out_h || !b->registered || scan < 0 || scan >= b->n_scans || which < 0 || which > 4) return LMONO_EINVAL;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int n = 0;
    const float4 *src = nullptr;
    int fn[4];
    HIP_TRY(c, hipMemcpy(fn, b->v.feat_n + scan * 4, sizeof(fn), hipMemcpyDeviceToHost));
    switch (which) {
    case 0: HIP_TRY(c, hipMemcpy(&n, b->v.n_cloud + scan, sizeof(int), hipMemcpyDeviceToHost)); src = b->v.cloud + b->off_h[scan]; break;
    case 1: n = fn[0]; src = b->v.sharp + (size_t)scan * kMaxSharp; break;
    case 2: n = fn[1]; src = b->v.less_sharp + (size_t)scan * kMaxLessSharp; break;
    case 3: n = fn[2]; src = b->v.flat + (size_t)scan * kMaxFlat; break;
    default: n = fn[3]; src = b->v.less_flat + b->off_h[scan]; break;
    }
    if (n > cap) { c->err = "get_cloud: output capacity too small"; return LMONO_ECAPACITY; }
    if (n > 0) HIP_TRY(c, hipMemcpy(out_h, src, sizeof(float4) * n, hipMemcpyDeviceToHost));
    return n;
}

extern "C" int lmono_batch_get_curvature(lmono_ctx *c, lmono_scan_batch *b, int scan, float *curv_h, int32_t *label_h, int cap)
{
    if (!c || !b || !b->registered || scan < 0 || scan >= b->n_scans) return LMONO_EINVAL;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int n = 0;
    HIP_TRY(c, hipMemcpy(&n, b->v.n_cloud + scan, sizeof(int), hipMemcpyDeviceToHost));
    if (n > cap) { c->err = "get_curvature: output capacity too small"; return LMONO_ECAPACITY; }
    if (curv_h && n > 0) {
        // no registration keeps the curvature: k_curvature runs here for the one scan, into a buffer of the accessor's own (grow_replace: the
        // stream is idle above and below)
        if (!b->mem.grow_replace(b->curv, b->curv_cap, (size_t)n, /*floor=*/1 << 17)) { c->err = "get_curvature: hipMalloc failed"; return LMONO_ENOMEM; }
        hipLaunchKernelGGL(k_curvature, dim3((n + kCurvTile - 1) / kCurvTile), dim3(256), 0, c->stream, b->v, scan, b->curv);
        if (int rc = check_launch(c, "k_curvature")) return rc;
        HIP_TRY(c, hipMemcpyAsync(curv_h, b->curv, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (label_h && n > 0) {
        std::vector<int8_t> tmp(n);
        HIP_TRY(c, hipMemcpy(tmp.data(), b->v.label + b->off_h[scan], n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) label_h[i] = tmp[i];
    }
    return n;
}

static int ensure_odom_ws(lmono_ctx *c, lmono_scan_batch *b, int n_chains)
{
    DevOwner &m = b->mem;
    // k_lm_solve<planes>'s scratch: sized for the calling context's instantiation (a batch may meet contexts that differ in it)
    const size_t lmrec_need = (size_t)(n_chains > b->chains_cap ? n_chains : b->chains_cap) * (4 - c->lm_planes) * kMaxQueries;
    if (lmrec_need > b->lmrec_cap) {
        if (!m.alloc(b->lmrec, lmrec_need)) { c->err = "odometry workspace: hipMalloc failed"; return LMONO_ENOMEM; }
        b->lmrec_cap = lmrec_need;
    }
    if (n_chains <= b->chains_cap) return LMONO_OK;
    // the grow_keep policy, sized by hand: exactly n_chains (no doubling), and the outgrown buffers stay owned until the batch is destroyed
    bool ok = m.alloc(b->state, (size_t)n_chains * 8) && m.alloc(b->corr, (size_t)n_chains * kMaxQueries * 4) &&
              m.alloc(b->lm_info, (size_t)n_chains * 4) && m.alloc(b->crec, (size_t)n_chains * kMaxQueries * 4) &&
              m.alloc(b->seed, (size_t)n_chains * kMaxQueries) && m.alloc(b->wl, 8 * ((size_t)n_chains * kMaxQueries + 1)) &&
              m.alloc(b->ws, (size_t)n_chains * 8) && m.alloc(b->resid_d, (size_t)n_chains) && m.alloc(b->rstat, (size_t)n_chains * 4) &&
              m.alloc(b->rcount, (size_t)n_chains + 2);
    if (!ok) { c->err = "odometry workspace: hipMalloc failed"; return LMONO_ENOMEM; }
    b->chains_cap = n_chains;
    return LMONO_OK;
}

// hash grids of a registered batch, for the searches that use them
static int ensure_grid(lmono_ctx *c, lmono_scan_batch *b)
{
    if (b->grid_built) return LMONO_OK;
#ifdef LMONO_DIAG_SEARCH
    hipLaunchKernelGGL(k_grid_build, dim3(b->n_scans, 1 + kGridPar), dim3(1024), kGridLds, c->stream, b->v);
    int rc = check_launch(c, "k_grid_build");
    if (rc) return rc;
    b->grid_built = true; b->v.has_grid = 1;
    return LMONO_OK;
#else
    c->err = "the hash-grid searches exist in the diagnostic build only (-DLMONO_DIAG_SEARCH)";
    return LMONO_EINVAL;
#endif
}

// Chain-group streams of a context: forks the library's group streams off the context stream, joins them again on every exit path.
struct GroupFork {
    lmono_ctx *c; int G, g_own; bool forked = false;
    GroupFork(lmono_ctx *c_, int G_, int g_own_) : c(c_), G(G_), g_own(g_own_) {}
    int fork()
    {
        if (G <= 1) return LMONO_OK;
        for (int g = g_own; g < G; g++)
            if (!c->gstream[g]) {
                // LMONO_ODOM_STREAM_PRIORITY=1 (measurement switch): the chain groups' streams at the highest priority, so that their short dependent
                // launches are dispatched ahead of another context's wide grids (a front end running beside the odometry)
                int lo = 0, hi = 0;
                if (c->odom_prio && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess) HIP_TRY(c, hipStreamCreateWithPriority(&c->gstream[g], hipStreamNonBlocking, hi));
                else HIP_TRY(c, hipStreamCreateWithFlags(&c->gstream[g], hipStreamNonBlocking));
            }
        for (int g = 0; g <= G && g < 9; g++) if (!c->gev[g]) HIP_TRY(c, hipEventCreateWithFlags(&c->gev[g], hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->gev[0], c->stream));
        forked = true;                           // from here on the group streams may carry work: join() must run
        for (int g = g_own; g < G; g++) HIP_TRY(c, hipStreamWaitEvent(c->gstream[g], c->gev[0], 0));
        return LMONO_OK;
    }
    // every forked stream is waited on by the context stream; if recording / waiting itself fails, the stream is synchronised instead,
    // so that nothing enqueued later (or the destruction of the batch) can overtake the group's kernels
    int join()
    {
        if (!forked) return LMONO_OK;
        forked = false;
        int rc = LMONO_OK;
        for (int g = g_own; g < G; g++) {
            if (hipEventRecord(c->gev[g + 1], c->gstream[g]) != hipSuccess || hipStreamWaitEvent(c->stream, c->gev[g + 1], 0) != hipSuccess) {
                (void)hipStreamSynchronize(c->gstream[g]);
                c->err = "odometry: joining a chain-group stream failed"; rc = LMONO_ENODEV;
            }
        }
        return rc;
    }
    ~GroupFork() { (void)join(); }
};

// number of chain groups a launch sequence over n_ch chains uses on this context
static int odom_groups(const lmono_ctx *c, int n_ch)
{
    constexpr int kMinChainsPerGroup = 32;
    int G = c->opt[LMONO_OPT_ODOM_STREAMS];
    G = G < 1 ? 1 : (G > 8 ? 8 : G);
    if (c->stream != nullptr && G > 3 && !c->many_queues) G = 3;      // (GPU_MAX_HW_QUEUES >= 8 in the environment: one hardware queue per stream anyway)
    while (G > 1 && n_ch / G < kMinChainsPerGroup) G--;      // a group below 32 chains cannot fill its share of the CUs
    if (c->opt[LMONO_OPT_CORR_TILE] != 3) G = 1;            // only the default search is grouped
    return G;
}

// Steps [step_a, step_b) x 2 outer iterations of the chains [0, n_ch) of view o (o.clist set: of the listed chains), in G chain groups.
// Chain groups: with LMONO_OPT_ODOM_STREAMS = G > 1 the chains are cut into G groups, each advancing on its own stream, so that
// one group's solve and the ragged tail of its search kernel run beside the other groups' searches.  A solve launch is one four-wave
// workgroup per chain, 64 CUs for a group of 64 chains, and 1.2 - 1.3 such launches are in flight over the main pass: what they leave of
// those CUs to the search is set by LDS and registers, not by wave slots.  k_lm_solve<0> takes 1.4 KB of LDS and 240 VGPRs, so four
// k_corr_flat workgroups (two 136-VGPR waves per SIMD) fit beside it; k_lm_solve<4> (144 KB of LDS) excludes the search from its CU.
// Group 0 carries the per-kernel events.  The runtime maps streams onto 4 hardware queues
// (GPU_MAX_HW_QUEUES): the null stream on one of its own, created streams round-robin on the other three.  So the default context
// (null stream) runs group 0 on the null stream + 3 group streams = 4 distinct queues; a context on a caller-created stream runs
// at most 3 groups, all on the library's own streams (4 created streams would put two groups on one queue: 64-70 instead of 51 ms
// per step measured), and the caller's stream only forks and joins.
static int odom_launch_steps(lmono_ctx *c, lmono_scan_batch *b, const OdomView &o, int n_ch, int step_a, int step_b, int G, EvSet *es, int *ne)
{
    const int tile = c->opt[LMONO_OPT_CORR_TILE];
    hipStream_t st = c->stream;
    const int g_own = st == nullptr ? 1 : 0;                  // first group that runs on a stream of the library
    const size_t wl_stride = (size_t)b->chains_cap * kMaxQueries + 1;
    auto kev = [&](int i) -> hipEvent_t {
        if (!es) return nullptr;
        while ((int)es->kev.size() <= i) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; es->kev.push_back(e); }
        return es->kev[i];
    };
    GroupFork fork(c, G, g_own);
    int rc = fork.fork();
    if (rc) return rc;
    for (int step = step_a; step < step_b; step++) {
        for (int outer = 0; outer < 2; outer++) {
            for (int g = 0; g < G; g++) {
                hipStream_t sg = (G == 1 || g < g_own) ? st : c->gstream[g];
                OdomView og = o;
                og.chain0 = (int)((long long)g * n_ch / G); og.chain1 = (int)((long long)(g + 1) * n_ch / G);
                const int ng = og.chain1 - og.chain0;
                if (ng <= 0) continue;
                unsigned int *wlg = b->wl + g * wl_stride;
                hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
                if (g == 0 && es) { e0 = kev(*ne); e1 = kev(*ne + 1); e2 = kev(*ne + 2); }
                if (e0 && e1 && e2) (void)hipEventRecord(e0, sg);
                if (tile == 3) {
                    hipLaunchKernelGGL(k_corr_flat, dim3(8 * ((ng + 7) / 8) * kCfBlocks), dim3(kCfT), 0, sg, b->v, og, step, outer, wlg, c->opt[LMONO_OPT_DEFER_EVERY], c->stats_d);
                    hipLaunchKernelGGL(k_correspond_list, dim3(kListGrid), dim3(256), 0, sg, b->v, og, step, outer, (const unsigned int *)wlg, c->stats_d);
                }
#ifdef LMONO_DIAG_SEARCH
                else
                    hipLaunchKernelGGL(k_correspond, dim3(8 * ((ng + 7) / 8) * kCorrBlocks), dim3(256), 0, sg, b->v, og, step, outer);
#endif
                if (e0 && e1 && e2) (void)hipEventRecord(e1, sg);
                unsigned int *wlr = tile ? wlg : (unsigned int *)nullptr;
                if (c->lm_planes == 4) hipLaunchKernelGGL(k_lm_solve<4>, dim3(ng), dim3(kLmT), lm_rec_lds(4), sg, b->v, og, step, outer, wlr);
                else hipLaunchKernelGGL(k_lm_solve<0>, dim3(ng), dim3(kLmT), lm_rec_lds(0), sg, b->v, og, step, outer, wlr);
                if (e0 && e1 && e2) { (void)hipEventRecord(e2, sg); *ne += 3; }
            }
        }
    }
    return fork.join();
}

// Boundary validation + repair rounds of the chained schedule ("self-validating chains").  ext: incr[first - 1]
// was supplied by the caller (previous rank's last increment).  Synchronises the context stream (the flagged count decides what is
// launched).  Results in b->brep / b->resid_h / b->rerun_h.
static int odom_validate(lmono_ctx *c, lmono_scan_batch *b, OdomView o, bool ext, bool first_call, EvSet *es = nullptr, int *ne = nullptr)
{
    hipStream_t st = c->stream;
    const int n_chains = o.n_chains;
    lmono_boundary_report &R = b->brep;
    if (first_call) {
        R = lmono_boundary_report{};
        R.n_chains = n_chains; R.tol = o.tol;
        b->resid_h.assign(n_chains, 0.0); b->rerun_h.assign(n_chains, 0);
    }
    if (!b->rep_ev[0]) for (auto &e : b->rep_ev) HIP_TRY(c, hipEventCreate(&e));
    HIP_TRY(c, hipEventRecord(b->rep_ev[0], st));
    int max_len = 0;
    for (int ch = 0; ch < n_chains; ch++) { int s, e; chain_bounds(o.first, o.n_scans, n_chains, ch, s, e); max_len = e - s > max_len ? e - s : max_len; }
    const int tile = c->opt[LMONO_OPT_CORR_TILE];
    std::vector<int> rs((size_t)n_chains * 4);
    const int max_rounds = n_chains + 1;
    int still_flagged = 0;               // boundaries the LAST check of the loop flagged (non-zero only when the round cap ends the loop)
    for (int round = 0; round <= max_rounds; round++) {
        const bool very_first = first_call && round == 0;
        hipLaunchKernelGGL(k_boundary_check, dim3(1), dim3(256), 0, st, o, very_first ? b->resid_d : (double *)nullptr, very_first ? 1 : 0, ext ? 1 : 0);
        unsigned int cnt[2] = { 0, 0 };
        HIP_TRY(c, hipMemcpyAsync(cnt, b->rcount, sizeof(cnt), hipMemcpyDeviceToHost, st));
        if (very_first) HIP_TRY(c, hipMemcpyAsync(b->resid_h.data(), b->resid_d, sizeof(double) * n_chains, hipMemcpyDeviceToHost, st));     // both copies on the
        HIP_TRY(c, hipStreamSynchronize(st));                                                                                                 // context stream, one wait
        if (very_first) {
            for (int ch = 0; ch < n_chains; ch++) R.max_resid = b->resid_h[ch] > R.max_resid ? b->resid_h[ch] : R.max_resid;
            // boundary_residual() answers 1e300 for a NaN increment: no repair can make such a boundary agree -- report it instead of re-running
            // its chain in every round
            if (R.max_resid >= 1e299) { c->err = "odometry: a chain boundary holds a NaN increment (a scan pair without a usable solution)"; return LMONO_ESCAN; }
        }
        const int nf = (int)cnt[0];
        still_flagged = nf;
        if (nf == 0 || round == max_rounds) break;      // the check behind the last allowed round only counts what is left
        R.flagged += nf; R.rounds += 1;
        OdomView orp = o;
        orp.repair = 1; orp.clist = (const int *)(b->rcount + 2); orp.lead_full = -1;
        const int G = odom_groups(c, nf);
        if (tile) for (int g = 0; g < G; g++) HIP_TRY(c, hipMemsetAsync(b->wl + g * ((size_t)b->chains_cap * kMaxQueries + 1), 0, sizeof(unsigned int), st));
        // a repair chain usually agrees with the stored increments after a few pairs: launch in chunks, ask the device how many still run
        int done = 0, chunk = 3;          // 3, 6, 8, 8 ...: most chains agree after 2-4 pairs, the slowest after ~9 (2, 4, 8 launched 14 steps for those 9)
        while (done < max_len) {
            const int upto = done + chunk < max_len ? done + chunk : max_len;
            orp.step0 = 0;
            int rc = odom_launch_steps(c, b, orp, nf, done, upto, G, es, ne);      // group 0's repair launches are timed like the main pass's
            if (rc) return rc;
            done = upto;
            HIP_TRY(c, hipMemcpyAsync(cnt, b->rcount, sizeof(cnt), hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipStreamSynchronize(st));
            if (cnt[1] == 0) break;
            chunk = chunk < 8 ? chunk * 2 : 8;
        }
    }
    HIP_TRY(c, hipEventRecord(b->rep_ev[1], st));
    HIP_TRY(c, hipMemcpyAsync(rs.data(), b->rstat, sizeof(int) * 4 * n_chains, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, b->rep_ev[0], b->rep_ev[1]) == hipSuccess) R.repair_ms += ms;
    R.pairs_rerun = 0; R.chains_rerun = 0;
    R.unresolved = still_flagged;        // boundaries above the tolerance after the last round (0 unless the round cap ended the loop)
    for (int ch = 0; ch < n_chains; ch++) {
        b->rerun_h[ch] = rs[ch * 4 + 1];
        R.pairs_rerun += rs[ch * 4 + 1]; R.chains_rerun += rs[ch * 4 + 3] > 0 ? 1 : 0;
    }
    return check_launch(c, "boundary validation");
}

static OdomView odom_view(lmono_ctx *c, lmono_scan_batch *b, int n_chains, int lead, int first)
{
    OdomView o{};
    o.n_scans = b->n_scans; o.n_chains = n_chains; o.lead = lead; o.first = first; o.fixed_k = -1; o.chain0 = 0; o.chain1 = n_chains;
    o.lead_full = c->opt[LMONO_OPT_CORR_TILE] == 3 ? c->opt[LMONO_OPT_LEAD_FULL] : -1;     // only the default search thins lead-in pairs
    o.state = b->state; o.corr = b->corr; o.incr = b->incr; o.lm_info = b->lm_info; o.crec = b->crec; o.lmrec = b->lmrec; o.seed = b->seed;
    o.ws = b->ws; o.repair = 0; o.step0 = 0; o.clist = nullptr; o.rstat = b->rstat; o.rcount = b->rcount;
    o.tol = 1e-9 * (double)c->opt[LMONO_OPT_BOUNDARY_TOL];
    return o;
}

static int odom_run(lmono_ctx *c, lmono_scan_batch *b, int n_chains, int lead, int first, double *incr_d, double *poses_d, bool want_poses, bool validate = true)
{
    if (!c || !b || !b->registered || lead < 0 || first < 0 || first >= b->n_scans) return LMONO_EINVAL;
    const int n = b->n_scans;
    if (n_chains < 1) n_chains = 1;
    if (n_chains > n - first) n_chains = n - first;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_odom_ws(c, b, n_chains);
    if (rc) return rc;
    OdomView o = odom_view(c, b, n_chains, lead, first);
    b->last_chains = n_chains; b->last_lead = lead; b->last_first = first;
    int max_steps = 0;
    for (int ch = 0; ch < n_chains; ch++) {
        int s, e;
        chain_bounds(first, n, n_chains, ch, s, e);
        const int begin = s - lead > 0 ? s - lead : 0;
        const int steps = e - begin - 1;
        max_steps = steps > max_steps ? steps : max_steps;
    }
    hipStream_t st = c->stream;
    if (c->n_sets == 0 || c->sets[c->n_sets - 1].odom) c->ev = c->next_set();
    if (!c->ev) { c->err = "hipEventCreate failed"; return LMONO_ENODEV; }
    c->sets[c->n_sets - 1].odom = true;
    HIP_TRY(c, hipEventRecord(c->ev[8], st));
    const int ninit = n > n_chains ? n : n_chains;
    hipLaunchKernelGGL(k_odom_init, dim3((ninit + 255) / 256), dim3(256), 0, st, o);
    const int tile = c->opt[LMONO_OPT_CORR_TILE];
    if (tile != 3) { rc = ensure_grid(c, b); if (rc) return rc; }
    const int G = odom_groups(c, n_chains);
    if (tile) for (int g = 0; g < G; g++) HIP_TRY(c, hipMemsetAsync(b->wl + g * ((size_t)b->chains_cap * kMaxQueries + 1), 0, sizeof(unsigned int), st));
    EvSet &es = c->sets[c->n_sets - 1];
    int ne = 0;
    if (c->opt[LMONO_OPT_LEAD_SEED] > 0 && n_chains > 2 && lead >= 3 && max_steps > 1 && o.ws) {
        // the first step of every chain, then the lead-in states are re-seeded from the neighbouring chains' first results (k_lead_seed_median)
        rc = odom_launch_steps(c, b, o, n_chains, 0, 1, G, &es, &ne);
        if (rc) return rc;
        hipLaunchKernelGGL(k_lead_seed_median, dim3((n_chains + 255) / 256), dim3(256), 0, st, o);
        hipLaunchKernelGGL(k_lead_seed_apply, dim3((n_chains + 255) / 256), dim3(256), 0, st, o);
        rc = odom_launch_steps(c, b, o, n_chains, 1, max_steps, G, &es, &ne);
    } else
        rc = odom_launch_steps(c, b, o, n_chains, 0, max_steps, G, &es, &ne);
    if (rc) return rc;
    es.n_kev = ne;
    // the chained schedule validates itself: every chain's warm start against its predecessor's last increment, repair where they differ
    b->brep = lmono_boundary_report{};
    b->brep.n_chains = n_chains;
    b->resid_h.assign((size_t)n_chains, 0.0); b->rerun_h.assign((size_t)n_chains, 0);      // a run without validation reports zeros, not the previous layout's values
    // (the repair launches carry no per-kernel events: the correspondence / solve sums of lmono_timing_read are the main pass's; the
    // repair's device time is lmono_boundary_report.repair_ms)
    b->validation_pending = !validate;
    if (validate && o.tol > 0.0 && n_chains > 1) { rc = odom_validate(c, b, o, false, true); if (rc) return rc; }
    if (want_poses) hipLaunchKernelGGL(k_pose_prefix, dim3(1), dim3(64), 0, st, (const double *)b->incr, b->poses, first, n);
    HIP_TRY(c, hipEventRecord(c->ev[9], st));
    rc = check_launch(c, "odometry kernels");
    if (rc) return rc;
    if (incr_d) HIP_TRY(c, hipMemcpyAsync(incr_d, b->incr, sizeof(double) * 7 * n, hipMemcpyDeviceToDevice, st));
    if (poses_d) HIP_TRY(c, hipMemcpyAsync(poses_d, b->poses, sizeof(double) * 7 * (n - first), hipMemcpyDeviceToDevice, st));
    return LMONO_OK;
}

extern "C" int lmono_odom_batch_d(lmono_ctx *c, lmono_scan_batch *b, int n_chains, int lead, double *incr_d, double *poses_d)
{
    return odom_run(c, b, n_chains, lead, 0, incr_d, poses_d, poses_d != nullptr);
}

extern "C" int lmono_odom_shard_d(lmono_ctx *c, lmono_scan_batch *b, int n_chains, int lead, int first_owned, double *incr_d)
{
    return odom_run(c, b, n_chains, lead, first_owned, incr_d, nullptr, false);
}

extern "C" int lmono_odom_shard_main_d(lmono_ctx *c, lmono_scan_batch *b, int n_chains, int lead, int first_owned, double *incr_d)
{
    return odom_run(c, b, n_chains, lead, first_owned, incr_d, nullptr, false, false);
}

extern "C" int lmono_odom_shard_validate(lmono_ctx *c, lmono_scan_batch *b, const double *prev_incr_h, double *incr_d, int *changed_last)
{
    if (!c || !b || !b->registered || b->last_chains < 1 || (prev_incr_h && b->last_first < 1)) return LMONO_EINVAL;
    if (!prev_incr_h && !b->validation_pending) return LMONO_EINVAL;     // without an external boundary there is only the deferred validation to run
    HIP_TRY(c, hipSetDevice(c->device));
    OdomView o = odom_view(c, b, b->last_chains, b->last_lead, b->last_first);
    const int n = b->n_scans;
    double before[7], after[7];
    // every copy below is ordered on the context stream (a blocking hipMemcpy would wait for whatever another context has queued on the null stream)
    HIP_TRY(c, hipMemcpyAsync(before, b->incr + (size_t)(n - 1) * 7, sizeof(before), hipMemcpyDeviceToHost, c->stream));
    if (prev_incr_h) HIP_TRY(c, hipMemcpyAsync(b->incr + (size_t)(o.first - 1) * 7, prev_incr_h, sizeof(double) * 7, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // after lmono_odom_shard_main_d this is the batch's ONE validation: the rank boundary (chain 0) goes through the same repair rounds as the
    // chain boundaries inside the rank instead of a second tail of sequential steps behind them
    const bool first_call = b->validation_pending;
    b->validation_pending = false;
    if (first_call) { b->brep = lmono_boundary_report{}; b->brep.n_chains = b->last_chains; b->resid_h.assign((size_t)b->last_chains, 0.0); b->rerun_h.assign((size_t)b->last_chains, 0); }
    if (o.tol > 0.0 && (prev_incr_h || b->last_chains > 1)) { int rc = odom_validate(c, b, o, prev_incr_h != nullptr, first_call); if (rc) return rc; }
    HIP_TRY(c, hipMemcpyAsync(after, b->incr + (size_t)(n - 1) * 7, sizeof(after), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (changed_last) *changed_last = std::memcmp(before, after, sizeof(before)) != 0 ? 1 : 0;
    if (incr_d) HIP_TRY(c, hipMemcpyAsync(incr_d, b->incr, sizeof(double) * 7 * n, hipMemcpyDeviceToDevice, c->stream));
    return LMONO_OK;
}

extern "C" int lmono_odom_boundary_report(lmono_ctx *c, lmono_scan_batch *b, lmono_boundary_report *rep, double *resid_h, int32_t *rerun_h, int cap)
{
    if (!c || !b || !rep) return LMONO_EINVAL;
    *rep = b->brep;
    const int n = b->brep.n_chains;
    if ((resid_h || rerun_h) && cap < n) { c->err = "boundary_report: output capacity too small"; return LMONO_ECAPACITY; }
    for (int i = 0; i < n && i < (int)b->resid_h.size(); i++) { if (resid_h) resid_h[i] = b->resid_h[i]; if (rerun_h) rerun_h[i] = b->rerun_h[i]; }
    return LMONO_OK;
}

extern "C" int lmono_odom_batch(lmono_ctx *c, lmono_scan_batch *b, int n_chains, int lead, double *incr_h, double *poses_h)
{
    int rc = odom_run(c, b, n_chains, lead, 0, nullptr, nullptr, poses_h != nullptr);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int n = b->n_scans;
    if (incr_h) HIP_TRY(c, hipMemcpy(incr_h, b->incr, sizeof(double) * 7 * n, hipMemcpyDeviceToHost));
    if (poses_h) HIP_TRY(c, hipMemcpy(poses_h, b->poses, sizeof(double) * 7 * n, hipMemcpyDeviceToHost));
    return LMONO_OK;
}

// ---- online laserOdometry: one scan per call (A-LOAM's node callbacks) -------------------------------------------------------------
// A stream owns a batch of history + 1 fixed-size slots.  Scan t is registered into the slot behind scan t - 1's (the raw points are
// copied into the slot, the rest of the slot is NaN: scanRegistration drops NaN points first), so "last" = the previous slot keeps its
// feature clouds and (line, azimuth bin) index from the previous call; one chain, pinned to the new slot, runs the scan pair from the
// stream's para_q / para_t.  When the slots run out, the last slot's "last" data move to slot 0 and the cycle restarts at slot 1.
struct lmono_odom_stream {
    lmono_ctx *ctx = nullptr;
    lmono_scan_batch *batch = nullptr;
    float *in_d = nullptr;
    DevOwner mem;
    int cap_pts = 0, n_slots = 0, slot = 0;
    long long frame = 0;
    double para[8] = { 0, 0, 0, 1, 0, 0, 0, 0 };       // q_last_curr (x y z w), t_last_curr
    double q_w[4] = { 0, 0, 0, 1 }, t_w[3] = { 0, 0, 0 };
};

extern "C" void lmono_odom_stream_destroy(lmono_odom_stream *s)
{
    if (!s) return;
    if (s->batch) lmono_batch_destroy(s->batch);
    delete s;
}

extern "C" lmono_odom_stream *lmono_odom_stream_create(lmono_ctx *c, int max_points, int n_lines, float min_range, int history)
{
    if (!c || max_points <= 0 || history < 1 || (n_lines != 16 && n_lines != 32 && n_lines != 64)) return nullptr;
    if (c->opt[LMONO_OPT_CORR_TILE] != 3) { c->err = "lmono_odom_stream: needs the default correspondence search (LMONO_OPT_CORR_TILE 3)"; return nullptr; }
    if (hipSetDevice(c->device) != hipSuccess) return nullptr;
    lmono_odom_stream *s = new lmono_odom_stream();
    s->ctx = c; s->cap_pts = max_points; s->n_slots = history + 1;
    s->batch = lmono_batch_create(c, s->n_slots, (int64_t)s->n_slots * max_points);
    if (!s->batch || !s->mem.alloc(s->in_d, (size_t)s->n_slots * max_points * 4)) { c->err = "lmono_odom_stream_create: allocation failed"; lmono_odom_stream_destroy(s); return nullptr; }
    lmono_scan_batch *b = s->batch;
    b->off_h.resize(s->n_slots + 1);
    for (int i = 0; i <= s->n_slots; i++) b->off_h[i] = (int64_t)i * max_points;
    b->n_scans = s->n_slots; b->total = (int64_t)s->n_slots * max_points; b->max_pts = max_points;
    BatchView &v = b->v;
    v.in = (const float4 *)s->in_d; v.n_scans = s->n_slots; v.scan0 = 0; v.n_lines = n_lines; v.min_range = min_range; v.has_grid = 0;
    bool ok = hipMemcpy(b->off_d, b->off_h.data(), sizeof(int64_t) * (s->n_slots + 1), hipMemcpyHostToDevice) == hipSuccess;
    // empty slots: no points, no features
    ok = ok && hipMemset(s->in_d, 0xff, (size_t)s->n_slots * max_points * 16) == hipSuccess;
    ok = ok && hipMemset(v.n_cloud, 0, sizeof(int) * s->n_slots) == hipSuccess && hipMemset(v.feat_n, 0, sizeof(int) * 4 * s->n_slots) == hipSuccess;
    ok = ok && hipMemset(v.status, 0, sizeof(int) * s->n_slots) == hipSuccess;
    ok = ok && ensure_odom_ws(c, b, 1) == LMONO_OK;
    if (!ok) { c->err = "lmono_odom_stream_create: initialisation failed"; lmono_odom_stream_destroy(s); return nullptr; }
    b->registered = true;
    return s;
}

// everything of slot `from` that a scan pair reads of its "last" scan, copied to slot `to`
static int stream_copy_last(lmono_ctx *c, lmono_scan_batch *b, int from, int to)
{
    hipStream_t st = c->stream;
    BatchView &v = b->v;
    const int64_t of = b->off_h[from], ot = b->off_h[to];
    const size_t P = (size_t)(b->off_h[1] - b->off_h[0]);
#define CP(arr, stride, off_from, off_to) HIP_TRY(c, hipMemcpyAsync((arr) + (off_to), (arr) + (off_from), sizeof(*(arr)) * (stride), hipMemcpyDeviceToDevice, st))
    CP(v.feat_n, 4, (size_t)from * 4, (size_t)to * 4);
    CP(v.n_cloud, 1, (size_t)from, (size_t)to);
    CP(v.status, 1, (size_t)from, (size_t)to);
    CP(v.less_sharp, kMaxLessSharp, (size_t)from * kMaxLessSharp, (size_t)to * kMaxLessSharp);
    CP(v.less_flat, P, (size_t)of, (size_t)ot);
    CP(v.lbc_pts, kMaxLessSharp, (size_t)from * kMaxLessSharp, (size_t)to * kMaxLessSharp);
    CP(v.lbs_pts, P, (size_t)of, (size_t)ot);
    CP(v.lb_start, 2 * (kLineKeys + 1), (size_t)from * 2 * (kLineKeys + 1), (size_t)to * 2 * (kLineKeys + 1));
    CP(v.lb_elev, 2 * 66, (size_t)from * 2 * 66, (size_t)to * 2 * 66);
    CP(v.line_first_ge, 2 * 66, (size_t)from * 2 * 66, (size_t)to * 2 * 66);
    CP(v.line_last_le, 2 * 66, (size_t)from * 2 * 66, (size_t)to * 2 * 66);
#undef CP
    return LMONO_OK;
}

extern "C" int lmono_odom_step(lmono_ctx *c, lmono_odom_stream *s, const float *xyzi, int n_points, int on_device, int use_warm_start,
                               double *q_last_curr, double *t_last_curr, double *q_w_curr, double *t_w_curr, int32_t *info)
{
    if (!c || !s || s->ctx != c || !xyzi || n_points < 0) return LMONO_EINVAL;
    if (n_points > s->cap_pts) { c->err = "lmono_odom_step: more points than the stream's slots hold"; return LMONO_ECAPACITY; }
    if (use_warm_start && (!q_last_curr || !t_last_curr)) return LMONO_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    lmono_scan_batch *b = s->batch;
    hipStream_t st = c->stream;
    int next = s->frame == 0 ? 1 : s->slot + 1;
    if (next >= s->n_slots) {
        int rc = stream_copy_last(c, b, s->slot, 0);
        if (rc) return rc;
        next = 1;
    }
    float *dst = s->in_d + (size_t)next * s->cap_pts * 4;
    if (n_points > 0) HIP_TRY(c, hipMemcpyAsync(dst, xyzi, (size_t)n_points * 16, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if (n_points < s->cap_pts) HIP_TRY(c, hipMemsetAsync(dst + (size_t)n_points * 4, 0xff, (size_t)(s->cap_pts - n_points) * 16, st));
    int rc = scanreg_launch(c, b, next, 1, n_points, n_points > 0 ? n_points : 1);
    if (rc) return rc;
    b->feat_h.clear();
    int iters[4] = { 0, 0, 0, 0 };
    if (s->frame > 0) {
        if (use_warm_start) { for (int i = 0; i < 4; i++) s->para[i] = q_last_curr[i]; for (int i = 0; i < 3; i++) s->para[4 + i] = t_last_curr[i]; }
        HIP_TRY(c, hipMemcpyAsync(b->state, s->para, sizeof(double) * 8, hipMemcpyHostToDevice, st));
        OdomView o = odom_view(c, b, 1, 0, 0);
        o.fixed_k = next; o.ws = nullptr; o.lead_full = -1;
        HIP_TRY(c, hipMemsetAsync(b->wl, 0, sizeof(unsigned int), st));
        rc = odom_launch_steps(c, b, o, 1, 0, 1, 1, nullptr, nullptr);
        if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync(s->para, b->state, sizeof(double) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(iters, b->lm_info, sizeof(iters), hipMemcpyDeviceToHost, st));
    }
    int fn[6] = { 0, 0, 0, 0, 0, 0 };
    HIP_TRY(c, hipMemcpyAsync(fn, b->v.n_cloud + next, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(fn + 1, b->v.feat_n + next * 4, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(fn + 5, b->v.status + next, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (s->frame > 0) {
        // laserOdometry's accumulation: t_w_curr += q_w_curr * t_last_curr; q_w_curr = q_w_curr * q_last_curr
        const double *q = s->para, *t = s->para + 4;
        const double ux = s->q_w[0], uy = s->q_w[1], uz = s->q_w[2], w = s->q_w[3];
        const double uvx = 2.0 * (uy * t[2] - uz * t[1]), uvy = 2.0 * (uz * t[0] - ux * t[2]), uvz = 2.0 * (ux * t[1] - uy * t[0]);
        s->t_w[0] += t[0] + w * uvx + (uy * uvz - uz * uvy);
        s->t_w[1] += t[1] + w * uvy + (uz * uvx - ux * uvz);
        s->t_w[2] += t[2] + w * uvz + (ux * uvy - uy * uvx);
        const double bx = q[0], by = q[1], bz = q[2], bw = q[3];
        const double nw = w * bw - ux * bx - uy * by - uz * bz, nx = w * bx + ux * bw + uy * bz - uz * by;
        const double ny = w * by + uy * bw + uz * bx - ux * bz, nz = w * bz + uz * bw + ux * by - uy * bx;
        s->q_w[0] = nx; s->q_w[1] = ny; s->q_w[2] = nz; s->q_w[3] = nw;
    }
    if (q_last_curr) for (int i = 0; i < 4; i++) q_last_curr[i] = s->para[i];
    if (t_last_curr) for (int i = 0; i < 3; i++) t_last_curr[i] = s->para[4 + i];
    if (q_w_curr) for (int i = 0; i < 4; i++) q_w_curr[i] = s->q_w[i];
    if (t_w_curr) for (int i = 0; i < 3; i++) t_w_curr[i] = s->t_w[i];
    if (info) { for (int i = 0; i < 6; i++) info[i] = fn[i]; info[6] = (iters[0] << 8) | iters[1]; info[7] = iters[3]; }
    s->slot = next; s->frame++;
    if (fn[5] & kStatusRingOverflow) { c->err = "lmono_odom_step: a ring holds more than LMONO_RING_CAP points"; return LMONO_ESCAN; }
    return LMONO_OK;
}

extern "C" int lmono_odom_stream_scan(lmono_odom_stream *s, lmono_scan_batch **batch, int *scan)
{
    if (!s || s->frame == 0) return LMONO_EINVAL;
    if (batch) *batch = s->batch;
    if (scan) *scan = s->slot;
    return LMONO_OK;
}

extern "C" int lmono_odom_correspond(lmono_ctx *c, lmono_scan_batch *b, int scan, const double q[4], const double t[3],
                                     int32_t *corr_h, int cap)
{
    if (!c || !b || !b->registered || scan < 1 || scan >= b->n_scans || !q || !t || !corr_h) return LMONO_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    double x[8] = { q[0], q[1], q[2], q[3], t[0], t[1], t[2], 0.0 };
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(b->xq, x, sizeof(x), hipMemcpyHostToDevice));
    int fn[4];
    HIP_TRY(c, hipMemcpy(fn, b->v.feat_n + scan * 4, sizeof(fn), hipMemcpyDeviceToHost));
    const int nq = fn[0] + fn[2];
    if (nq > cap) { c->err = "odom_correspond: output capacity too small"; return LMONO_ECAPACITY; }
    OdomView o{};
    o.n_scans = b->n_scans; o.n_chains = 1; o.lead = 0; o.fixed_k = scan; o.chain0 = 0; o.chain1 = 1; o.lead_full = -1;
    o.state = b->xq; o.corr = b->corr_pair; o.incr = nullptr; o.lm_info = nullptr; o.crec = b->crec_pair; o.seed = nullptr;
    int rc;
    if (c->opt[LMONO_OPT_CORR_TILE] != 3) { rc = ensure_grid(c, b); if (rc) return rc; }
    if (c->opt[LMONO_OPT_CORR_TILE]) {
        rc = ensure_odom_ws(c, b, 1);
        if (rc) return rc;
        HIP_TRY(c, hipMemsetAsync(b->wl, 0, sizeof(unsigned int), c->stream));
        hipLaunchKernelGGL(k_corr_flat, dim3(8 * kCfBlocks), dim3(kCfT), 0, c->stream, b->v, o, 0, 0, b->wl, c->opt[LMONO_OPT_DEFER_EVERY], c->stats_d);
        hipLaunchKernelGGL(k_correspond_list, dim3(kListGrid), dim3(256), 0, c->stream, b->v, o, 0, 0, (const unsigned int *)b->wl, c->stats_d);
    }
#ifdef LMONO_DIAG_SEARCH
    else
        hipLaunchKernelGGL(k_correspond, dim3(8 * kCorrBlocks), dim3(256), 0, c->stream, b->v, o, 0, 0);
#endif
    rc = check_launch(c, "k_correspond");
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (nq > 0) HIP_TRY(c, hipMemcpy(corr_h, b->corr_pair, sizeof(int) * 4 * nq, hipMemcpyDeviceToHost));
    return nq;
}

extern "C" int lmono_pose_prefix_d(lmono_ctx *c, const double *incr_d, int first, int n, double *poses_d)
{
    if (!c || !incr_d || !poses_d || first < 0 || n <= first) return LMONO_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_pose_prefix, dim3(1), dim3(64), 0, c->stream, incr_d, poses_d, first, n);
    return check_launch(c, "k_pose_prefix");
}

extern "C" int lmono_pose_rebase_d(lmono_ctx *c, const double *bases_d, int n_bases, double *poses_d, int n)
{
    if (!c || !poses_d || n <= 0 || n_bases < 0 || (n_bases > 0 && !bases_d)) return LMONO_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_pose_rebase, dim3((n + 255) / 256), dim3(256), 0, c->stream, bases_d, n_bases, poses_d, n);
    return check_launch(c, "k_pose_rebase");
}
