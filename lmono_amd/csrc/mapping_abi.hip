// mapping_abi.hip -- C ABI of laserMapping: map refine, voxel filter and the mapper over mapping.hip (included by lmono_hip.hip after lidar_abi.hip)
#pragma once
// ---- scan-to-map optimisation step of laserMapping, batched over independent streams ------------------------
extern "C" int lmono_map_refine(lmono_ctx *c, int n_streams,
                                const float *corner_map_h, const int64_t *corner_map_off, const float *surf_map_h, const int64_t *surf_map_off,
                                const float *corner_stack_h, const int64_t *corner_stack_off, const float *surf_stack_h, const int64_t *surf_stack_off,
                                double *pose_qt, int32_t *stats_h, int32_t *nn_out_h)
{
    if (!c || n_streams <= 0 || !corner_map_off || !surf_map_off || !corner_stack_off || !surf_stack_off || !pose_qt) return LMONO_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t tot[4] = { corner_map_off[n_streams], surf_map_off[n_streams], corner_stack_off[n_streams], surf_stack_off[n_streams] };
    const float *src_h[4] = { corner_map_h, surf_map_h, corner_stack_h, surf_stack_h };
    for (int k = 0; k < 4; k++) if (tot[k] < 0 || (tot[k] > 0 && !src_h[k])) return LMONO_EINVAL;
    DevBuf db(c);
    bool ok = true;
    float4 *cloud_d[4];
    for (int k = 0; k < 4; k++) cloud_d[k] = (float4 *)db.up(src_h[k], (size_t)tot[k] * 4, ok);
    // hash tables, cell-sorted copies and scratch of the 2 n_streams map clouds
    std::vector<int64_t> toff((size_t)2 * n_streams + 1, 0);
    for (int s = 0; s < n_streams; s++)
        for (int w = 0; w < 2; w++) {
            const int64_t n = (w ? surf_map_off : corner_map_off)[s + 1] - (w ? surf_map_off : corner_map_off)[s];
            if (n < 0 || n > (1 << 24) - 2) { c->err = "lmono_map_refine: bad map cloud size"; return LMONO_EINVAL; }
            int T = 1024;
            while (T < n + 1) T <<= 1;
            toff[(size_t)2 * s + w + 1] = toff[(size_t)2 * s + w] + T;
        }
    GridCell *cells = (GridCell *)db.up((const char *)nullptr, (size_t)toff.back() * sizeof(GridCell), ok);
    float4 *sorted[2] = { (float4 *)db.up((const float *)nullptr, (size_t)tot[0] * 4, ok), (float4 *)db.up((const float *)nullptr, (size_t)tot[1] * 4, ok) };
    int *slot[2] = { db.up((const int *)nullptr, (size_t)tot[0], ok), db.up((const int *)nullptr, (size_t)tot[1], ok) };
    int *rank[2] = { db.up((const int *)nullptr, (size_t)tot[0], ok), db.up((const int *)nullptr, (size_t)tot[1], ok) };
    int *masks = db.up((const int *)nullptr, (size_t)4 * n_streams, ok);     // [2 n] masks, [2 n] run allocators
    const int64_t nq_total = tot[2] + tot[3];
    MapRec *rec = (MapRec *)db.up((const char *)nullptr, (size_t)(nq_total > 0 ? nq_total : 1) * sizeof(MapRec), ok);
    int *nn_d = nn_out_h ? db.up((const int *)nullptr, (size_t)(nq_total > 0 ? nq_total : 1) * 5, ok) : nullptr;
    int *nn_tmp_d = db.up((const int *)nullptr, (size_t)(nq_total > 0 ? nq_total : 1) * 5, ok);
    std::vector<double> xh((size_t)n_streams * 8, 0.0);
    for (int s = 0; s < n_streams; s++) for (int k = 0; k < 7; k++) xh[(size_t)s * 8 + k] = pose_qt[(size_t)s * 7 + k];
    double *x_d = db.up(xh.data(), xh.size(), ok);
    std::vector<int> zero((size_t)n_streams * 16, 0);
    int *stats_d = db.up(zero.data(), (size_t)n_streams * 8, ok);
    unsigned int *bar_d = (unsigned int *)db.up(zero.data(), (size_t)n_streams * 16, ok);          // cluster barriers of the two solves, zeroed
    double *part_d = db.up((const double *)nullptr, (size_t)n_streams * kMsEvals * kMsMaxK * 28, ok);
    db.ready(ok);
    if (!ok) { c->err = "lmono_map_refine: device allocation / upload failed"; return LMONO_ENOMEM; }
    std::vector<CloudJob> jobs((size_t)2 * n_streams);
    std::vector<MapStream> st((size_t)n_streams);
    int max_nq = 0, max_nmap = 0;
    int64_t rec_at = 0;
    for (int s = 0; s < n_streams; s++) {
        MapStream &S = st[(size_t)s];
        for (int w = 0; w < 2; w++) {
            const int64_t *moff = w ? surf_map_off : corner_map_off, *soff = w ? surf_stack_off : corner_stack_off;
            CloudJob &J = jobs[(size_t)2 * s + w];
            J.src = cloud_d[w] + moff[s]; J.n = (int)(moff[s + 1] - moff[s]);
            max_nmap = std::max(max_nmap, J.n);
            J.cell = cells + toff[(size_t)2 * s + w]; J.tcap = (int)(toff[(size_t)2 * s + w + 1] - toff[(size_t)2 * s + w]);
            J.sorted = sorted[w] + moff[s]; J.slot_of = slot[w] + moff[s]; J.rank_of = rank[w] + moff[s];
            J.mask_out = masks + 2 * s + w; J.bump = masks + 2 * n_streams + 2 * s + w;
            S.cell[w] = J.cell; S.sorted[w] = J.sorted; S.cloud[w] = J.src; S.mask[w] = J.mask_out; S.n_map[w] = J.n;
            S.stack[w] = cloud_d[2 + w] + soff[s]; S.n_stack[w] = (int)(soff[s + 1] - soff[s]);
        }
        S.rec = rec + rec_at; S.x = x_d + (size_t)s * 8; S.stats = stats_d + (size_t)s * 8;
        S.part = part_d + (size_t)s * kMsEvals * kMsMaxK * 28; S.bar = bar_d + (size_t)s * 16;
        S.nn_out = nn_d ? nn_d + rec_at * 5 : nullptr;
        S.nn_tmp = nn_tmp_d + rec_at * 5;
        const int nq = S.n_stack[0] + S.n_stack[1];
        rec_at += nq;
        max_nq = nq > max_nq ? nq : max_nq;
    }
    CloudJob *jobs_d = db.up(jobs.data(), jobs.size(), ok);
    MapStream *st_d = db.up(st.data(), st.size(), ok);
    db.ready(ok);
    if (!ok) { c->err = "lmono_map_refine: device allocation / upload failed"; return LMONO_ENOMEM; }
    hipStream_t stream = c->stream;
    struct Events {             // destroyed on every return path
        hipEvent_t e[3] = { nullptr, nullptr, nullptr };
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } evs;
    for (hipEvent_t &x : evs.e) if (hipEventCreate(&x) != hipSuccess) { c->err = "hipEventCreate failed"; return LMONO_ENODEV; }
    const hipEvent_t ev0 = evs.e[0], ev1 = evs.e[1], ev2 = evs.e[2];
    (void)hipEventRecord(ev0, stream);
    launch_cloud_grids(stream, (const CloudJob *)jobs_d, 2 * n_streams, max_nmap);
    (void)hipEventRecord(ev1, stream);
    for (int outer = 0; outer < 2; outer++) {
        if (max_nq > 0) {
            hipLaunchKernelGGL(k_map_correspond, dim3((max_nq + 7) / 8, n_streams), dim3(256), 0, stream, (const MapStream *)st_d, outer, 0, n_streams);
            hipLaunchKernelGGL(k_map_factor, dim3((max_nq + 63) / 64, n_streams), dim3(64), 0, stream, (const MapStream *)st_d, outer, 0, n_streams);
        }
        launch_map_solve(stream, (const MapStream *)st_d, n_streams, outer, c->map_budget);
    }
    (void)hipEventRecord(ev2, stream);
    int rc = check_launch(c, "map refine kernels");
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(stream));
    float ms_grid = 0.f, ms_opt = 0.f;
    (void)hipEventElapsedTime(&ms_grid, ev0, ev1); (void)hipEventElapsedTime(&ms_opt, ev1, ev2);
    HIP_TRY(c, hipMemcpy(xh.data(), x_d, sizeof(double) * xh.size(), hipMemcpyDeviceToHost));
    for (int s = 0; s < n_streams; s++) for (int k = 0; k < 7; k++) pose_qt[(size_t)s * 7 + k] = xh[(size_t)s * 8 + k];
    {
        std::vector<int> sh((size_t)n_streams * 8);
        HIP_TRY(c, hipMemcpy(sh.data(), stats_d, sizeof(int) * sh.size(), hipMemcpyDeviceToHost));
        for (int s = 0; s < n_streams; s++) if (sh[(size_t)s * 8 + 6]) { c->err = "lmono_map_refine: a solve's cluster barrier timed out"; return LMONO_ENODEV; }
    }
    if (stats_h) {
        HIP_TRY(c, hipMemcpy(stats_h, stats_d, sizeof(int) * (size_t)n_streams * 8, hipMemcpyDeviceToHost));
        // device time of the whole batch in microseconds: grid build, then the two correspond + solve rounds
        for (int s = 0; s < n_streams; s++) { stats_h[(size_t)s * 8 + 6] = (int)(ms_grid * 1e3f); stats_h[(size_t)s * 8 + 7] = (int)(ms_opt * 1e3f); }
    }
    if (nn_out_h && nq_total > 0) HIP_TRY(c, hipMemcpy(nn_out_h, nn_d, sizeof(int) * (size_t)nq_total * 5, hipMemcpyDeviceToHost));
    return LMONO_OK;
}

// ---- pcl::VoxelGrid on arbitrary clouds (laserMapping's scan and cube filters), a batch of clouds per call -----------------
extern "C" int lmono_voxel_filter(lmono_ctx *c, int n_clouds, const float *xyzi_h, const int64_t *off, const float *leaf_h,
                                  float *out_h, int64_t *out_off)
{
    if (!c || n_clouds <= 0 || !off || !leaf_h || !out_h || !out_off) return LMONO_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t total = off[n_clouds];
    if (off[0] != 0 || total < 0 || (total > 0 && !xyzi_h)) return LMONO_EINVAL;
    for (int k = 0; k < n_clouds; k++) {
        const int64_t n = off[k + 1] - off[k];
        if (n < 0 || n > kVoxCloudMax) { c->err = "lmono_voxel_filter: a cloud holds more than 65536 points"; return LMONO_ECAPACITY; }
        if (!(leaf_h[k] > 0.f)) { c->err = "lmono_voxel_filter: leaf size must be positive"; return LMONO_EINVAL; }
    }
    DevBuf db(c);
    bool ok = true;
    float4 *in_d = (float4 *)db.up(xyzi_h, (size_t)total * 4, ok);
    float4 *out_d = (float4 *)db.up((const float *)nullptr, (size_t)total * 4, ok);
    unsigned int *ka = db.up((const unsigned int *)nullptr, (size_t)total, ok), *kb = db.up((const unsigned int *)nullptr, (size_t)total, ok);
    int *ia = db.up((const int *)nullptr, (size_t)total, ok), *ib = db.up((const int *)nullptr, (size_t)total, ok);
    int *nout_d = db.up((const int *)nullptr, (size_t)n_clouds, ok);
    size_t ws_total = 0;
    for (int k = 0; k < n_clouds; k++) ws_total += vox_ws_ints(off[k + 1] - off[k]);
    int *ws_d = db.up((const int *)nullptr, ws_total, ok);
    std::vector<VoxJob> jobs((size_t)n_clouds);
    size_t ws_at = 0;
    for (int k = 0; k < n_clouds; k++) {
        VoxJob &J = jobs[(size_t)k];
        J.ws = ws_d + ws_at; ws_at += vox_ws_ints(off[k + 1] - off[k]);
        J.in = in_d + off[k]; J.n = (int)(off[k + 1] - off[k]); J.inv_leaf = 1.0f / leaf_h[k];
        J.out = out_d + off[k]; J.n_out = nout_d + k;
        J.key_a = ka + off[k]; J.key_b = kb + off[k]; J.idx_a = ia + off[k]; J.idx_b = ib + off[k];
    }
    VoxJob *jobs_d = db.up(jobs.data(), jobs.size(), ok);
    std::vector<int> tab;
    vox_tile_table(jobs.data(), jobs.size(), tab);
    int *tab_d = db.up(tab.data(), tab.size(), ok);
    db.ready(ok);
    if (!ok) { c->err = "lmono_voxel_filter: device allocation / upload failed"; return LMONO_ENOMEM; }
    launch_voxel_jobs(c->stream, (const VoxJob *)jobs_d, tab_d, (int)tab.size(), 4);
    int rc = check_launch(c, "voxel filter kernels");
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<int> nout((size_t)n_clouds);
    HIP_TRY(c, hipMemcpy(nout.data(), nout_d, sizeof(int) * (size_t)n_clouds, hipMemcpyDeviceToHost));
    out_off[0] = 0;
    for (int k = 0; k < n_clouds; k++) {
        if (nout[(size_t)k] < 0) { c->err = "lmono_voxel_filter: kernel rejected a cloud"; return LMONO_ECAPACITY; }
        out_off[k + 1] = out_off[k] + nout[(size_t)k];
        if (nout[(size_t)k] > 0)
            HIP_TRY(c, hipMemcpy(out_h + 4 * out_off[k], out_d + off[k], sizeof(float) * 4 * (size_t)nout[(size_t)k], hipMemcpyDeviceToHost));
    }
    return LMONO_OK;
}

// ---- laserMapping with a device-resident cube map -------------------------------------------------------------
// The 21 x 21 x 11 cube array of laserMapping.cpp lives in two HBM arenas (corner, surf); the host keeps, per cube, only
// (offset, count).  Per frame the scan's feature clouds are taken from the scan batch in HBM, every numeric step runs in
// the kernels above, and what crosses PCIe is the pose (56 B), the cube index of every down-sampled scan point and the
// sizes of the re-filtered cubes.
namespace {
constexpr int kMapW = 21, kMapH = 21, kMapD = 11, kMapCubes = kMapW * kMapH * kMapD;
constexpr int64_t kMapArena = 6 << 20;        // points per arena half
constexpr int kMapNeighMax = 1 << 20;         // map points of the cube neighbourhood handed to one optimisation
constexpr int kMapStackMax = kVoxCloudMax;
struct Seg { int64_t off = 0; int n = 0; };
}
struct lmono_mapper {
    lmono_ctx *ctx = nullptr;
    float leaf[2] = { 0.4f, 0.8f };
    int cen[3] = { 10, 10, 5 };
    double q_wmap_wodom[4] = { 0, 0, 0, 1 }, t_wmap_wodom[3] = { 0, 0, 0 };
    std::vector<Seg> cube[2];
    DevOwner mem;                               // device buffers and the pinned mail boxes
    int *pin_i = nullptr; double *pin_x = nullptr; int *pin_cube = nullptr; int *pin_nout = nullptr; char *pin_blob = nullptr;
    size_t pin_i_cap = 0, pin_x_cap = 0, pin_cube_cap = 0, pin_nout_cap = 0, pin_blob_cap = 0;
    float4 *arena[2][2] = { { nullptr, nullptr }, { nullptr, nullptr } };   // [type][half]
    int half[2] = { 0, 0 };
    int64_t bump[2] = { 0, 0 };
    // per-frame workspace
    float4 *stack[2] = { nullptr, nullptr }, *newpts[2] = { nullptr, nullptr }, *neigh[2] = { nullptr, nullptr }, *sorted[2] = { nullptr, nullptr }, *cat[2] = { nullptr, nullptr };
    unsigned int *vk[2] = { nullptr, nullptr };
    hipStream_t side = nullptr;                 // second stream of a frame: the neighbourhood gather + grids run beside the scan clouds' voxel filter
    hipEvent_t ev_side = nullptr, ev_sizes = nullptr;
    double *solve_part = nullptr;               // k_map_solve's cluster: partial sums [kMsEvals][kMsMaxK][28]
    int *vws[2] = { nullptr, nullptr };         // voxel filter workspace (vox_ws_ints per job), vws_cap ints each
    size_t vws_cap = 0;
    int *vi[2] = { nullptr, nullptr }, *slot[2] = { nullptr, nullptr }, *rank[2] = { nullptr, nullptr }, *cube_of[2] = { nullptr, nullptr }, *pos[2] = { nullptr, nullptr };
    GridCell *cells[2] = { nullptr, nullptr };
    int tcap = 0;
    int *masks = nullptr, *nout = nullptr, *stats = nullptr;
    int *nout_big = nullptr;        // output sizes of the cube filter jobs of a batched call (owned by the first mapper)
    size_t nout_cap = 0;
    // contiguous mail boxes of a batched call (owned by the first mapper, grown on demand): poses, counters, cube indices /
    // placements of all streams travel in one copy per phase
    int *cubebuf = nullptr;
    size_t cubebuf_cap = 0;
    double *x = nullptr;
    MapRec *rec = nullptr;
    int *nn_tmp = nullptr;          // [2 kMapStackMax][5]
    void *jobs = nullptr;           // device scratch for job arrays
    size_t jobs_bytes = 0;
    MapStream *stream_d = nullptr;
    // device-resident bookkeeping (lmono_mapper_process; the batched entry keeps the tables on the host and converts on entry)
    bool dev_mode = false;
    MapDev *dev = nullptr;
    MapUpd *upd = nullptr;
    char *fblob[2] = { nullptr, nullptr };      // a frame's control block + job tables on the device, by frame parity
    char *fstage[2] = { nullptr, nullptr };     // their pinned staging buffers
    int parity = 0;
    unsigned int *vk_s[2] = { nullptr, nullptr };   // the scan filter's own workspace (it runs beside the previous frame's map update)
    int *vi_s[2] = { nullptr, nullptr }, *vws_s[2] = { nullptr, nullptr };
    int *cube_of_d = nullptr;
    hipEvent_t ev_commit = nullptr, ev_assign = nullptr, ev_pose = nullptr, ev_solve = nullptr;
    char *pin_back = nullptr;                   // pinned: the frame's read-back
    int bump_seen[2] = { 0, 0 }, nmap_seen[2] = { 0, 0 };
};

extern "C" void lmono_mapper_destroy(lmono_mapper *m)
{
    if (!m) return;
    if (m->ctx) (void)hipStreamSynchronize(m->ctx->stream);
    if (m->side) { (void)hipStreamSynchronize(m->side); (void)hipStreamDestroy(m->side); }
    if (m->ev_side) (void)hipEventDestroy(m->ev_side);
    if (m->ev_sizes) (void)hipEventDestroy(m->ev_sizes);
    for (hipEvent_t e : { m->ev_commit, m->ev_assign, m->ev_pose, m->ev_solve }) if (e) (void)hipEventDestroy(e);
    delete m;                   // its memory goes last
}

extern "C" lmono_mapper *lmono_mapper_create(lmono_ctx *c, float line_res, float plane_res)
{
    if (!c || !(line_res > 0.f) || !(plane_res > 0.f)) return nullptr;
    if (hipSetDevice(c->device) != hipSuccess) return nullptr;
    lmono_mapper *m = new lmono_mapper();
    m->ctx = c; m->leaf[0] = line_res; m->leaf[1] = plane_res;
    m->cube[0].assign((size_t)kMapCubes, Seg()); m->cube[1].assign((size_t)kMapCubes, Seg());
    m->tcap = 1;
    m->vws_cap = (size_t)128 * kVxHdr + (size_t)((kMapNeighMax + kMapStackMax) / kVxTile + 128) * kVxWsTile;     // <= 75 cube jobs per type and frame
    while (m->tcap < kMapNeighMax + 1) m->tcap <<= 1;
    bool ok = true;
    for (int t = 0; t < 2 && ok; t++) {
        ok = ok && m->mem.alloc(m->arena[t][0], (size_t)kMapArena) && m->mem.alloc(m->arena[t][1], (size_t)kMapArena) &&
             m->mem.alloc(m->stack[t], (size_t)kMapStackMax) && m->mem.alloc(m->newpts[t], (size_t)kMapStackMax) &&
             m->mem.alloc(m->neigh[t], (size_t)kMapNeighMax) && m->mem.alloc(m->sorted[t], (size_t)kMapNeighMax) &&
             m->mem.alloc(m->cat[t], (size_t)kMapNeighMax + kMapStackMax) &&
             m->mem.alloc(m->vk[t], (size_t)2 * (kMapNeighMax + kMapStackMax)) && m->mem.alloc(m->vi[t], (size_t)2 * (kMapNeighMax + kMapStackMax)) &&
             m->mem.alloc(m->slot[t], (size_t)kMapNeighMax) && m->mem.alloc(m->rank[t], (size_t)kMapNeighMax) &&
             m->mem.alloc(m->cube_of[t], (size_t)kMapStackMax) && m->mem.alloc(m->pos[t], (size_t)kMapStackMax) &&
             m->mem.alloc(m->cells[t], (size_t)m->tcap) && m->mem.alloc(m->vws[t], m->vws_cap);
    }
    m->jobs_bytes = 1 << 20;
    m->nout_cap = 1024;
    ok = ok && m->mem.alloc(m->masks, 4) && m->mem.alloc(m->nout, 2 * 256) && m->mem.alloc(m->nout_big, m->nout_cap) && m->mem.alloc(m->stats, 8) && m->mem.alloc(m->x, 8) &&
         m->mem.alloc(m->rec, (size_t)2 * kMapStackMax) && m->mem.alloc(m->nn_tmp, (size_t)10 * kMapStackMax) && m->mem.alloc((char *&)m->jobs, m->jobs_bytes) && m->mem.alloc(m->stream_d, 1) &&
         m->mem.alloc(m->solve_part, (size_t)kMsEvals * kMsMaxK * 28);
    ok = ok && hipStreamCreateWithFlags(&m->side, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&m->ev_side, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&m->ev_sizes, hipEventDisableTiming) == hipSuccess;
    constexpr size_t kFrameBlob = 4096;
    ok = ok && m->mem.alloc(m->dev, 1) && m->mem.alloc(m->upd, 1) && m->mem.alloc(m->fblob[0], kFrameBlob) && m->mem.alloc(m->fblob[1], kFrameBlob) && m->mem.alloc(m->cube_of_d, (size_t)2 * kMapStackMax);
    for (int t = 0; t < 2 && ok; t++)
        ok = ok && m->mem.alloc(m->vk_s[t], (size_t)2 * kMapStackMax) && m->mem.alloc(m->vi_s[t], (size_t)2 * kMapStackMax) && m->mem.alloc(m->vws_s[t], vox_ws_ints(kMapStackMax));
    for (hipEvent_t *e : { &m->ev_commit, &m->ev_assign, &m->ev_pose, &m->ev_solve }) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    if (ok && (ok = m->mem.pinned(m->fstage[0], 2 * kFrameBlob + 256))) { m->fstage[1] = m->fstage[0] + kFrameBlob; m->pin_back = m->fstage[0] + 2 * kFrameBlob; }
    if (!ok) { c->err = "lmono_mapper_create: device allocation failed"; lmono_mapper_destroy(m); return nullptr; }
    return m;
}

extern "C" int lmono_mapper_reset(lmono_ctx *c, lmono_mapper *m)
{
    if (!c || !m) return LMONO_EINVAL;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipStreamSynchronize(m->side));
    m->dev_mode = false;          // the (empty) table goes back to the device with the next lmono_mapper_process
    m->bump_seen[0] = m->bump_seen[1] = 0; m->nmap_seen[0] = m->nmap_seen[1] = 0;
    for (int t = 0; t < 2; t++) { m->cube[(size_t)t].assign((size_t)kMapCubes, Seg()); m->half[t] = 0; m->bump[t] = 0; }
    m->cen[0] = 10; m->cen[1] = 10; m->cen[2] = 5;
    m->q_wmap_wodom[0] = m->q_wmap_wodom[1] = m->q_wmap_wodom[2] = 0.0; m->q_wmap_wodom[3] = 1.0;
    m->t_wmap_wodom[0] = m->t_wmap_wodom[1] = m->t_wmap_wodom[2] = 0.0;
    return LMONO_OK;
}

// compaction: copy every live segment of one type into the other arena half
static int mapper_compact(lmono_mapper *m, int t)
{
    lmono_ctx *c = m->ctx;
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // rare path: the frame's tables in the job scratch are done with before it is overwritten
    std::vector<CopyJob> jobs;
    const int nh = m->half[t] ^ 1;
    int64_t at = 0;
    for (Seg &s : m->cube[(size_t)t]) {
        if (s.n == 0) continue;
        jobs.push_back({ m->arena[t][m->half[t]] + s.off, m->arena[t][nh] + at, s.n });
        s.off = at; at += s.n;
    }
    if (jobs.size() * sizeof(CopyJob) > m->jobs_bytes) { c->err = "lmono_mapper: job scratch too small"; return LMONO_ECAPACITY; }
    if (!jobs.empty()) {
        HIP_TRY(c, hipMemcpyAsync(m->jobs, jobs.data(), jobs.size() * sizeof(CopyJob), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_copy_jobs, dim3((unsigned)jobs.size()), dim3(256), 0, c->stream, (const CopyJob *)m->jobs);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    m->half[t] = nh; m->bump[t] = at;
    return LMONO_OK;
}

namespace {
template <typename T> int mp_grow(lmono_ctx *c, lmono_mapper *m, T *&p, size_t &cap, size_t need)
{
    if (!m->mem.grow_keep(p, cap, need, /*floor=*/1024)) { c->err = "lmono_mapper: allocation failed"; return LMONO_ENOMEM; }     // kept: kernels in flight may still read the old buffer
    return LMONO_OK;
}
// pinned host mail boxes of the frame's read-backs (a copy into pageable memory holds the calling thread until it is done; into pinned memory it is
// asynchronous -- the host goes on enqueueing): grown on demand, freed with the mapper
template <typename T> int pin_grow(lmono_ctx *c, lmono_mapper *m, T *&p, size_t &cap, size_t need)
{
    if (!m->mem.grow_keep_pinned(p, cap, need, /*floor=*/1024)) { c->err = "lmono_mapper: pinned allocation failed"; return LMONO_ENOMEM; }
    return LMONO_OK;
}
// job tables of one phase for every stream go through one pinned-free staging path: a scratch device buffer owned by the
// first mapper of the call, grown on demand
// Every table of a call gets its OWN piece of the scratch (bump allocation, 256-B aligned): no phase waits for the previous phase's
// kernels to be done with "the" job table before it uploads its own (round 4: four stream synchronisations per frame less).  A scratch
// that runs out is replaced by a larger one; the old one stays allocated (kernels in flight still read it) until the mapper is destroyed.
struct JobScratch {
    lmono_mapper *owner;
    size_t used = 0;
    void *last = nullptr;        // device address of the table uploaded last
    // space for a table whose entries point into the table itself: place() it (its device address is `last`), fill it, send() it
    int place(lmono_ctx *c, size_t bytes)
    {
        used = (used + 255) & ~(size_t)255;
        if (used + bytes > owner->jobs_bytes) {
            size_t nb = owner->jobs_bytes;
            while (nb < bytes || nb < 2 * (used + bytes)) nb <<= 1;
            if (!owner->mem.alloc((char *&)owner->jobs, nb)) { c->err = "lmono_mapper: job scratch allocation failed"; return LMONO_ENOMEM; }      // keep mode: the old scratch stays owned
            owner->jobs_bytes = nb; used = 0;
        }
        last = (char *)owner->jobs + used;
        used += bytes;
        return LMONO_OK;
    }
    int send(lmono_ctx *c, const void *src, size_t bytes, hipStream_t st)
    {
        if (bytes > 0 && hipMemcpyAsync(last, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) { c->err = "lmono_mapper: job upload failed"; return LMONO_ENODEV; }
        return LMONO_OK;
    }
    int upload(lmono_ctx *c, const void *src, size_t bytes, hipStream_t st) { const int rc = place(c, bytes); return rc ? rc : send(c, src, bytes, st); }
};
// a copy of n points as jobs of at most kCopyChunk points: one workgroup per job, and a 16 k-point cube in one workgroup was a 12-us kernel
constexpr int kCopyChunk = 4096;
static inline void push_copy(std::vector<CopyJob> &jobs, const float4 *src, float4 *dst, int n)
{
    for (int at = 0; at < n; at += kCopyChunk) jobs.push_back({ src + at, dst + at, std::min(kCopyChunk, n - at) });
}
void mp_qrot(const double *q, const double *v, double *o)
{
    const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
    const double uvx = 2.0 * (uy * v[2] - uz * v[1]), uvy = 2.0 * (uz * v[0] - ux * v[2]), uvz = 2.0 * (ux * v[1] - uy * v[0]);
    o[0] = v[0] + w * uvx + (uy * uvz - uz * uvy); o[1] = v[1] + w * uvy + (uz * uvx - ux * uvz); o[2] = v[2] + w * uvz + (ux * uvy - uy * uvx);
}
void mp_qmul(const double *a, const double *bq, double *o)
{
    o[3] = a[3] * bq[3] - a[0] * bq[0] - a[1] * bq[1] - a[2] * bq[2];
    o[0] = a[3] * bq[0] + a[0] * bq[3] + a[1] * bq[2] - a[2] * bq[1];
    o[1] = a[3] * bq[1] + a[1] * bq[3] + a[2] * bq[0] - a[0] * bq[2];
    o[2] = a[3] * bq[2] + a[2] * bq[3] + a[0] * bq[1] - a[1] * bq[0];
}
int mp_cube_of(double v, int cen) { int q = (int)((v + 25.0) / 50.0) + cen; if (v + 25.0 < 0) q--; return q; }
void mp_shift(lmono_mapper *m, int axis, int dir)
{
    const int n[3] = { kMapW, kMapH, kMapD }, stride[3] = { 1, kMapW, kMapW * kMapH };
    const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
    for (int t = 0; t < 2; t++)
        for (int u = 0; u < n[a1]; u++)
            for (int v = 0; v < n[a2]; v++) {
                const int base = u * stride[a1] + v * stride[a2];
                std::vector<Seg> &arr = m->cube[(size_t)t];
                if (dir > 0) { for (int i = n[axis] - 1; i >= 1; i--) arr[(size_t)(base + i * stride[axis])] = arr[(size_t)(base + (i - 1) * stride[axis])]; arr[(size_t)base] = Seg(); }
                else { for (int i = 0; i < n[axis] - 1; i++) arr[(size_t)(base + i * stride[axis])] = arr[(size_t)(base + (i + 1) * stride[axis])]; arr[(size_t)(base + (n[axis] - 1) * stride[axis])] = Seg(); }
            }
}
// Host state of a mapper that lmono_mapper_process_batch changes; put back when the call fails after changing it.  The device
// side needs no undo: new points only ever land in free arena space (behind `bump`, or in the idle half during compaction).
struct MapperUndo {
    lmono_mapper *m;
    std::vector<Seg> cube[2];
    int cen[3], half[2];
    int64_t bump[2];
    double q[4], t[3];
    explicit MapperUndo(lmono_mapper *mp) : m(mp)
    {
        for (int k = 0; k < 2; k++) { cube[k] = m->cube[(size_t)k]; half[k] = m->half[k]; bump[k] = m->bump[k]; }
        for (int k = 0; k < 3; k++) { cen[k] = m->cen[k]; t[k] = m->t_wmap_wodom[k]; }
        for (int k = 0; k < 4; k++) q[k] = m->q_wmap_wodom[k];
    }
    void restore()
    {
        for (int k = 0; k < 2; k++) { m->cube[(size_t)k].swap(cube[k]); m->half[k] = half[k]; m->bump[k] = bump[k]; }
        for (int k = 0; k < 3; k++) { m->cen[k] = cen[k]; m->t_wmap_wodom[k] = t[k]; }
        for (int k = 0; k < 4; k++) m->q_wmap_wodom[k] = q[k];
    }
};
struct MapperUndoAll {
    std::vector<MapperUndo> u;
    bool committed = false;
    ~MapperUndoAll() { if (!committed) for (MapperUndo &x : u) x.restore(); }
};
struct FrameState {            // one stream's frame
    double x[8];
    std::vector<int> valid;
    int n_last[2], n_stack[2], n_map[2];
    const int *cube_h[2] = { nullptr, nullptr };       // cube index of every stack point: into the pinned read-back
};
inline size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }
// ---- the host steps of a laserMapping frame, shared by the frame with the cube table on the device (mapper_process_dev) and on the host (BatchCall)
// the feature counts [n_scans][4] of a scan batch on the host: fetched on first use after a registration
int scan_feat_counts(lmono_ctx *c, lmono_scan_batch *b)
{
    if (!b->feat_h.empty()) return LMONO_OK;
    b->feat_h.assign((size_t)b->n_scans * 4, 0);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(b->feat_h.data(), b->v.feat_n, sizeof(int) * 4 * (size_t)b->n_scans, hipMemcpyDeviceToHost));
    return LMONO_OK;
}
// transformAssociateToMap: x[8] = the odometry pose moved into the map frame, q(xyzw) t pad
void associate_to_map(const lmono_mapper *m, const double *q_wodom, const double *t_wodom, double *x)
{
    double tmp[3];
    mp_qmul(m->q_wmap_wodom, q_wodom, x);
    mp_qrot(m->q_wmap_wodom, t_wodom, tmp);
    for (int k = 0; k < 3; k++) x[4 + k] = tmp[k] + m->t_wmap_wodom[k];
    x[7] = 0.0;
}
// transformUpdate: the map <- odometry transform from the refined pose x
void transform_update(lmono_mapper *m, const double *x, const double *q_wodom, const double *t_wodom)
{
    const double n2 = q_wodom[0] * q_wodom[0] + q_wodom[1] * q_wodom[1] + q_wodom[2] * q_wodom[2] + q_wodom[3] * q_wodom[3];
    const double qi[4] = { -q_wodom[0] / n2, -q_wodom[1] / n2, -q_wodom[2] / n2, q_wodom[3] / n2 };
    double tmp[3];
    mp_qmul(x, qi, m->q_wmap_wodom);
    mp_qrot(m->q_wmap_wodom, t_wodom, tmp);
    for (int k = 0; k < 3; k++) m->t_wmap_wodom[k] = x[4 + k] - tmp[k];
}
// The cube pose x falls into and the shifts of the cube array that keep it three cubes inside: the centre `cen` and the centre cube `cc` behind the
// shifts, the shifts as (axis, dir) in the order they are made -- per axis the +1 shifts, then the -1 shifts (empty, unallocated, in almost every frame)
struct CentreCube { int cen[3], cc[3]; std::vector<std::pair<int, int>> shifts; };
CentreCube centre_cube(const double *x, const int *cen)
{
    const int dims[3] = { kMapW, kMapH, kMapD };
    CentreCube o;
    for (int a = 0; a < 3; a++) {
        o.cen[a] = cen[a]; o.cc[a] = mp_cube_of(x[4 + a], cen[a]);
        while (o.cc[a] < 3) { o.shifts.push_back({ a, +1 }); o.cc[a]++; o.cen[a]++; }
        while (o.cc[a] >= dims[a] - 3) { o.shifts.push_back({ a, -1 }); o.cc[a]--; o.cen[a]--; }
    }
    return o;
}
// the cubes of the 5 x 5 x 3 neighbourhood of cube cc that exist, in laserMapping's loop order (the layout of the gathered cloud): out[kMdValidMax], returns their number
int neighbourhood(const int *cc, int *out)
{
    int n = 0;
    for (int i = cc[0] - 2; i <= cc[0] + 2; i++)
        for (int j = cc[1] - 2; j <= cc[1] + 2; j++)
            for (int k = cc[2] - 1; k <= cc[2] + 1; k++)
                if (i >= 0 && i < kMapW && j >= 0 && j < kMapH && k >= 0 && k < kMapD) out[n++] = i + kMapW * j + kMapW * kMapH * k;
    return n;
}
// a cube is a 50 m box: at most 50 / leaf + 3 cells per axis, whatever it holds -> the passes the keys of its filter can need
int cube_filter_passes(float leaf)
{
    const double per_axis = 50.0 / (double)leaf + 3.0;
    int bits = 1;
    while (bits < 32 && std::ldexp(1.0, bits) < per_axis * per_axis * per_axis) bits++;
    return std::min(4, (bits + 8) / 9);
}
// VoxelGrid of the scan's cloud of type t, read in place from the scan batch; J.n (set first: the tile table needs it), workspaces and the count's address are the caller's
void scan_vox_job(VoxJob &J, const lmono_mapper *m, const lmono_scan_batch *b, int scan, int t, unsigned int *vk, int *vi, int *vws, int *n_out)
{
    J.in = t ? b->v.less_flat + b->off_h[(size_t)scan] : b->v.less_sharp + (size_t)scan * kMaxLessSharp;
    J.inv_leaf = 1.0f / m->leaf[t]; J.out = m->stack[t]; J.n_out = n_out;
    J.key_a = vk; J.key_b = vk + kMapStackMax; J.idx_a = vi; J.idx_b = vi + kMapStackMax; J.ws = vws;
}
// the grid of the neighbourhood cloud of type t (n points)
CloudJob neigh_cloud_job(const lmono_mapper *m, int t, int n)
{
    CloudJob J;
    J.src = m->neigh[t]; J.n = n; J.cell = m->cells[t]; J.tcap = m->tcap; J.sorted = m->sorted[t];
    J.slot_of = m->slot[t]; J.rank_of = m->rank[t]; J.mask_out = m->masks + t; J.bump = m->masks + 2 + t;
    return J;
}
// the optimisation's view of a mapper: the stack sizes are read from the device (n_stack_d), the map's too when n_map is null (k_map_gather_copy_clear writes them);
// pose, statistics and barrier counters live in the frame's block
MapStream map_stream(const lmono_mapper *m, const int *n_map, const int *n_stack_d, double *x, int *stats, unsigned int *bar)
{
    MapStream S;
    memset(&S, 0, sizeof(S));
    for (int t = 0; t < 2; t++) {
        S.cell[t] = m->cells[t]; S.sorted[t] = m->sorted[t]; S.cloud[t] = m->neigh[t]; S.mask[t] = m->masks + t; S.n_map[t] = n_map ? n_map[t] : 0;
        S.stack[t] = m->stack[t]; S.n_stack[t] = 0;
    }
    S.n_stack_d = n_stack_d; S.rec = m->rec; S.x = x; S.stats = stats; S.nn_out = nullptr; S.nn_tmp = m->nn_tmp;
    S.part = m->solve_part; S.bar = bar;
    return S;
}
// the optimisation, 2 x [correspond + factors + solve], of na streams of at most max_nq scan points each before the filter, enqueued at once
void launch_map_optimise(hipStream_t st, const MapStream *S_d, int na, int max_nq, int budget)
{
    // the filter keeps a fraction of a scan cloud: a quarter of the bound's blocks (at least 2048 / na per stream while few streams run) stride over the rest
    const int per_stream = std::max(1, std::max((max_nq + 31) / 32, std::min((max_nq + 7) / 8, 2048 / na))), per_f = std::max(1, (per_stream + 7) / 8);
    // (from 8 streams on: every stream's workgroups on one XCD -- map_block_of; LMONO_MAP_XCD=0: the 2-D launch, for measurements)
    static const bool xcd_off = [] { const char *e = getenv("LMONO_MAP_XCD"); return e && atoi(e) == 0; }();
    int nx_c = 0, nx_f = 0;
    const dim3 g_c = xcd_off ? dim3((unsigned)per_stream, (unsigned)na) : map_stream_grid(per_stream, na, nx_c);
    const dim3 g_f = xcd_off ? dim3((unsigned)per_f, (unsigned)na) : map_stream_grid(per_f, na, nx_f);
    for (int outer = 0; outer < 2; outer++) {
        if (max_nq > 0) {
            hipLaunchKernelGGL(k_map_correspond, g_c, dim3(256), 0, st, S_d, outer, nx_c, na);
            hipLaunchKernelGGL(k_map_factor, g_f, dim3(64), 0, st, S_d, outer, nx_f, na);
        }
        launch_map_solve(st, S_d, na, outer, budget);
    }
}
}

// ---- the cube table on the device (lmono_mapper_process) or on the host (lmono_mapper_process_batch, compaction): converted when the other side needs it
static int mapper_tables_to_host(lmono_ctx *c, lmono_mapper *m)
{
    if (!m->dev_mode) return LMONO_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipStreamSynchronize(m->side));
    std::vector<int2> tab((size_t)2 * kMapCubes);
    int tail[6];
    HIP_TRY(c, hipMemcpy(tab.data(), &m->dev->tab[0][0], sizeof(int2) * tab.size(), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(tail, &m->dev->bump[0], sizeof(tail), hipMemcpyDeviceToHost));
    for (int t = 0; t < 2; t++) {
        for (int k = 0; k < kMapCubes; k++) { Seg &sg = m->cube[(size_t)t][(size_t)k]; sg.off = tab[(size_t)t * kMapCubes + k].x; sg.n = tab[(size_t)t * kMapCubes + k].y; }
        m->bump[t] = tail[t];
    }
    m->dev_mode = false;
    if (tail[2]) { c->err = "lmono_mapper: a map update on the device was refused (capacity)"; return LMONO_ECAPACITY; }
    return LMONO_OK;
}
static int mapper_tables_to_device(lmono_ctx *c, lmono_mapper *m)
{
    if (m->dev_mode) return LMONO_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<int2> tab((size_t)2 * kMapCubes);
    for (int t = 0; t < 2; t++)
        for (int k = 0; k < kMapCubes; k++) { const Seg &sg = m->cube[(size_t)t][(size_t)k]; tab[(size_t)t * kMapCubes + k] = make_int2((int)sg.off, sg.n); }
    HIP_TRY(c, hipMemcpy(&m->dev->tab[0][0], tab.data(), sizeof(int2) * tab.size(), hipMemcpyHostToDevice));
    int tail[6] = { (int)m->bump[0], (int)m->bump[1], 0, 0, 0, 0 };
    HIP_TRY(c, hipMemcpy(&m->dev->bump[0], tail, sizeof(tail), hipMemcpyHostToDevice));
    const CloudJob cj[2] = { neigh_cloud_job(m, 0, 0), neigh_cloud_job(m, 1, 0) };
    HIP_TRY(c, hipMemcpy(&m->dev->cj[0], cj, sizeof(cj), hipMemcpyHostToDevice));
    m->bump_seen[0] = (int)m->bump[0]; m->bump_seen[1] = (int)m->bump[1];
    m->dev_mode = true;
    return LMONO_OK;
}

// One frame of one mapper with the bookkeeping on the device.  Streams: `side` takes the frame's upload, the scan clouds' voxel filter (beside the
// previous frame's map update, which is still running on the main stream), then -- behind that update's commit -- the shift of the cube array, the
// neighbourhood gather and its grids; the main stream takes the optimisation, hands the pose to the host, and goes on with the cube assignment, the
// update's plan, its copies and filters and the commit while the caller already prepares the next frame.
static int mapper_process_dev(lmono_ctx *c, lmono_mapper *m, lmono_scan_batch *b, int scan, const double *q_wodom, const double *t_wodom,
                              double *q_w_curr, double *t_w_curr, int32_t *stats_h)
{
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream, side = m->side;
    int rc;
    if ((rc = scan_feat_counts(c, b))) return rc;
    const int n_last[2] = { b->feat_h[(size_t)scan * 4 + 1], b->feat_h[(size_t)scan * 4 + 3] };
    if (n_last[0] > kMapStackMax || n_last[1] > kMapStackMax) { c->err = "lmono_mapper: scan cloud too large"; return LMONO_ECAPACITY; }
    // arena space: what the host saw last is two updates old; compact (on the host's copy of the table: rare) long before the bump pointer can reach the end
    static const int64_t compact_at = [] { const char *e = getenv("LMONO_MAP_COMPACT_AT"); return e ? (int64_t)atoll(e) : (int64_t)0; }();      // test hook: compact as soon as a
                                                                                                                                              // bump pointer has passed this many points
    for (int t = 0; t < 2; t++)
        if ((int64_t)m->bump_seen[t] + 2 * ((int64_t)m->nmap_seen[t] + 3 * kMapStackMax) + kMapStackMax > kMapArena || (compact_at > 0 && m->bump_seen[t] > compact_at)) {
            if ((rc = mapper_tables_to_host(c, m))) return rc;
            if ((rc = mapper_compact(m, t))) return rc;
        }
    if ((rc = mapper_tables_to_device(c, m))) return rc;
    // ---- host: transformAssociateToMap, centre cube, shifts (on copies: the mapper changes when the frame has succeeded)
    double x[8];
    associate_to_map(m, q_wodom, t_wodom, x);
    const CentreCube cu = centre_cube(x, m->cen);
    // ---- the frame's block: [MapFrame | VoxJob x 2 | tile table | MapStream | AssignJob x 2]
    const int par = m->parity;
    char *blob = m->fblob[par], *stage = m->fstage[par];
    VoxJob vj[2];
    vj[0].n = n_last[0]; vj[1].n = n_last[1];
    std::vector<int> tab;
    vox_tile_table(vj, 2, tab);
    const size_t o_vox = al16(sizeof(MapFrame)), o_tab = al16(o_vox + 2 * sizeof(VoxJob)), o_S = al16(o_tab + tab.size() * sizeof(int)), o_aj = al16(o_S + sizeof(MapStream)),
                 bytes = o_aj + 2 * sizeof(AssignJob);
    if (bytes > 4096) { c->err = "lmono_mapper: frame block too large"; return LMONO_ECAPACITY; }
    MapFrame *F_d = (MapFrame *)blob;
    memset(stage, 0, bytes);
    MapFrame *F = (MapFrame *)stage;
    for (int k = 0; k < 8; k++) F->x[k] = x[k];
    for (int k = 0; k < 3; k++) F->cen[k] = cu.cen[k];
    F->n_valid = neighbourhood(cu.cc, F->valid);
    for (int t = 0; t < 2; t++) scan_vox_job(vj[t], m, b, scan, t, m->vk_s[t], m->vi_s[t], m->vws_s[t], &F_d->n_stack[t]);
    memcpy(stage + o_vox, vj, sizeof(vj));
    if (!tab.empty()) memcpy(stage + o_tab, tab.data(), tab.size() * sizeof(int));
    const MapStream S = map_stream(m, nullptr, &F_d->n_stack[0], &F_d->x[0], &F_d->stats[0], &F_d->bar[0]);
    memcpy(stage + o_S, &S, sizeof(S));
    AssignJob aj[2];
    for (int t = 0; t < 2; t++) aj[t] = { m->stack[t], -1, &F_d->n_stack[0], t, &F_d->x[0], cu.cen[0], cu.cen[1], cu.cen[2], m->newpts[t], m->cube_of_d + (size_t)t * kMapStackMax };      // (n = -1: the job's own array of cube indices)
    memcpy(stage + o_aj, aj, sizeof(aj));
    MapDevCfg cfg;
    cfg.dev = m->dev; cfg.frame = F_d; cfg.upd = m->upd; cfg.S = (MapStream *)(blob + o_S);
    for (int t = 0; t < 2; t++) {
        cfg.arena[t] = m->arena[t][m->half[t]]; cfg.neigh[t] = m->neigh[t]; cfg.cat[t] = m->cat[t]; cfg.newpts[t] = m->newpts[t];
        cfg.vk[t] = m->vk[t]; cfg.vi[t] = m->vi[t]; cfg.vws[t] = m->vws[t]; cfg.inv_leaf[t] = 1.0f / m->leaf[t];
    }
    cfg.vws_cap = (int)m->vws_cap; cfg.cube_of[0] = m->cube_of_d; cfg.cube_of[1] = m->cube_of_d + kMapStackMax;
    // ---- side stream: upload, scan filter (behind the previous frame's cube assignment: it reads the stack), then behind the previous commit: shifts, gather, grids
    HIP_TRY(c, hipMemcpyAsync(blob, stage, bytes, hipMemcpyHostToDevice, side));
    HIP_TRY(c, hipStreamWaitEvent(side, m->ev_assign, 0));
    launch_voxel_jobs(side, (const VoxJob *)(blob + o_vox), (const int *)(blob + o_tab), (int)tab.size(), 4);
    HIP_TRY(c, hipStreamWaitEvent(side, m->ev_commit, 0));
    for (const std::pair<int, int> &sh : cu.shifts) {
        HIP_TRY(c, hipMemcpyAsync(&m->dev->tmp[0][0], &m->dev->tab[0][0], sizeof(int2) * 2 * kMapCubes, hipMemcpyDeviceToDevice, side));
        hipLaunchKernelGGL(k_map_shift, dim3((2 * kMapCubes + 255) / 256), dim3(256), 0, side, m->dev, sh.first, sh.second);
    }
    // the neighbourhood's plan, its copies and the emptied hash tables in one launch
    hipLaunchKernelGGL(k_map_gather_copy_clear, dim3(kMgcGrid), dim3(kMgcT), 0, side, cfg);
    {
        const int est = std::max(65536, std::max(m->nmap_seen[0], m->nmap_seen[1]) * 5 / 4 + 32768);
        launch_cloud_grids(side, (const CloudJob *)m->dev->cj, 2, est, true);
    }
    HIP_TRY(c, hipEventRecord(m->ev_side, side));
    // ---- main stream: the optimisation
    HIP_TRY(c, hipStreamWaitEvent(st, m->ev_side, 0));
    launch_map_optimise(st, (const MapStream *)(blob + o_S), 1, n_last[0] + n_last[1], c->map_budget);
    HIP_TRY(c, hipEventRecord(m->ev_solve, st));
    // the read-back leaves on the side stream (the main stream goes straight on): [x | stats | bar | n_stack | n_map | snap] of the frame -- snap = the map's
    // [bump | err | . | last_sum] as k_map_gather_copy_clear copied them at the head of this frame (the live words are rewritten by this frame's own
    // update on the main stream while the side stream reads; the snapshot is the previous update's, whole, as the header promises for stats[7])
    constexpr size_t kBackA = sizeof(double) * 8 + sizeof(int) * 8 + sizeof(unsigned int) * 16 + sizeof(int) * 4;
    static_assert(offsetof(MapFrame, snap) == kBackA, "the frame's read-back is one copy: x .. snap");
    HIP_TRY(c, hipStreamWaitEvent(side, m->ev_solve, 0));
    HIP_TRY(c, hipMemcpyAsync(m->pin_back, blob, kBackA + sizeof(int) * 6, hipMemcpyDeviceToHost, side));
    HIP_TRY(c, hipEventRecord(m->ev_pose, side));
    // ---- main stream: the scan joins the map
    {
        const int max_n = std::max(n_last[0], n_last[1]);
        if (max_n > 0) hipLaunchKernelGGL(k_map_assign, dim3((max_n + 255) / 256, 2), dim3(256), 0, st, (const AssignJob *)(blob + o_aj));
        HIP_TRY(c, hipEventRecord(m->ev_assign, st));
        // (k_map_assign's work inside the plan kernel -- one launch and one gap fewer in front of it -- was built and measured: 2.50-2.61 k frames/s against
        // 2.76-2.80 k; one compute unit transforming 11 k points costs more than the launch it saves)
        hipLaunchKernelGGL(k_map_plan_update, dim3(1), dim3(kMuT), 0, st, cfg);
        hipLaunchKernelGGL(k_copy_jobs_n, dim3(128), dim3(256), 0, st, (const CopyJob *)m->upd->copy, (const int *)&m->upd->n_copy);
        const int cube_passes = std::max(cube_filter_passes(m->leaf[0]), cube_filter_passes(m->leaf[1]));
        launch_voxel_jobs(st, (const VoxJob *)m->upd->vox, (const int *)m->upd->tiles, 160, cube_passes, (const int *)&m->upd->n_tiles);
        hipLaunchKernelGGL(k_map_commit, dim3(1 + 16), dim3(kMuH), 0, st, cfg);          // (workgroup 0 commits, the others do the plain copies)
        HIP_TRY(c, hipEventRecord(m->ev_commit, st));
    }
    m->parity ^= 1;
    for (int k = 0; k < 3; k++) m->cen[k] = cu.cen[k];          // the device's table has moved: so has the mapper's centre, whatever the frame's fate
    // ---- the one wait of the frame
    HIP_TRY(c, hipEventSynchronize(m->ev_pose));
    rc = check_launch(c, "mapper kernels");
    if (rc) return rc;
    const double *xb = (const double *)m->pin_back;
    const int *sb = (const int *)(m->pin_back + sizeof(double) * 8);
    const int *nb = (const int *)(m->pin_back + sizeof(double) * 8 + sizeof(int) * 8 + sizeof(unsigned int) * 16);
    const int *mb = (const int *)(m->pin_back + kBackA);
    if (sb[6]) { c->err = "lmono_mapper: a solve's cluster barrier timed out"; return LMONO_ENODEV; }
    if (nb[0] < 0 || nb[1] < 0) { c->err = "lmono_mapper: voxel filter rejected a scan cloud"; return LMONO_ECAPACITY; }
    if (mb[2]) { c->err = "lmono_mapper: the map update of an earlier frame was refused on the device (capacity)"; return LMONO_ECAPACITY; }
    for (int k = 0; k < 4; k++) q_w_curr[k] = xb[k];
    for (int k = 0; k < 3; k++) t_w_curr[k] = xb[4 + k];
    if (stats_h) {
        for (int k = 0; k < 6; k++) stats_h[k] = sb[k];
        stats_h[6] = nb[2] + nb[3];           // map points of the neighbourhood
        stats_h[7] = mb[4] + mb[5];           // points of the cubes the PREVIOUS frame's update rebuilt (this frame's update runs behind the return)
    }
    m->bump_seen[0] = mb[0]; m->bump_seen[1] = mb[1];
    m->nmap_seen[0] = nb[2]; m->nmap_seen[1] = nb[3];
    transform_update(m, xb, q_wodom, t_wodom);          // the shifts are the mapper's now
    return LMONO_OK;
}

// ---- n mappers (independent streams), each advanced by one frame with the cube tables on the host: every phase is one launch for all streams
namespace {
struct Touched { int s, t, ind, n_in; int64_t cat_off; bool filter; };      // a cube a frame's update rebuilds: [old points | new points in stack order]
struct PlanOut { std::vector<Touched> touched; std::vector<CopyJob> copy; const char *err = nullptr; };       // one stream's share of the update plan
struct SideGuard { hipStream_t s = nullptr; ~SideGuard() { if (s) (void)hipStreamSynchronize(s); } };       // no return path leaves work on the side stream behind
double tnow() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// One call of lmono_mapper_process_batch: its arguments, the streams' frames, what a phase leaves for the later ones, and the phases in the order they
// run.  The first mapper (m0) owns what the streams share: job scratch, pinned mail boxes, side stream and events.
struct BatchCall {
    lmono_ctx *c; int n; lmono_mapper *const *ms; lmono_scan_batch *const *bs; const int *scans;
    const double *q_wodom, *t_wodom; double *q_w_curr, *t_w_curr; int32_t *stats_h;
    lmono_mapper *m0; hipStream_t st, side;
    JobScratch js;
    std::vector<FrameState> F;
    MapperUndoAll undo;                      // every error return leaves the mappers as they were on entry
    // staging vectors of asynchronous copies live until the call returns (every path syncs the stream before that)
    std::vector<ScatterJob> sj;
    std::vector<char> vox_blob, side_blob;
    SideGuard side_guard;                    // (declared behind them: the side stream is waited for before they go)
    std::vector<int> act;                    // the streams whose map is large enough to optimise against
    double tp[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, tpa = 0, tpb = 0;      // LMONO_MAP_PROF
    int *ns_h = nullptr, *stats = nullptr;   // pinned: [n][2] filter counts; [n][8] statistics, behind ...
    double *xh = nullptr;                    // ... the pinned [n][8] poses
    const double *x_d = nullptr; const AssignJob *aj_d = nullptr;        // in the frame blob on the device: poses, assignment jobs
    std::vector<PlanOut> outs;               // the update: per-stream plans, then joined in stream order
    std::vector<Touched> touched;
    std::vector<CopyJob> copy, keep; std::vector<VoxJob> vox;
    std::vector<size_t> pos_at;              // [2 n] where the stack of (stream, type) starts among all stacks: in the cube indices, and in pos_all
    int *pos_all = nullptr;                  // pinned: the placement of every stack point in `cat`, at the head of the update's staging buffer
    size_t pos_total = 0, o_copy = 0, tables_cap = 0;       // all stack points; the update's tables behind their placements: where they start, and their bound
    int max_ns = 0;                          // the largest stack
    int host_phase(), gather_phase(), optimise_phase(), assign_phase(), plan_phase(), arena_phase(), update_phase();
    void results_phase(), plan_stream(int s, int tid);
};
// ---- phase 1 (host): transformAssociateToMap, centre cube, shifts, neighbourhood; scan cloud sizes
int BatchCall::host_phase()
{
    int rc;
    for (int s = 0; s < n; s++) if ((rc = scan_feat_counts(c, bs[s]))) return rc;
    for (int s = 0; s < n; s++) {
        lmono_mapper *m = ms[s];
        FrameState &f = F[(size_t)s];
        associate_to_map(m, q_wodom + 4 * s, t_wodom + 3 * s, f.x);
        const CentreCube cu = centre_cube(f.x, m->cen);
        for (const std::pair<int, int> &sh : cu.shifts) mp_shift(m, sh.first, sh.second);
        for (int k = 0; k < 3; k++) m->cen[k] = cu.cen[k];
        f.valid.resize((size_t)kMdValidMax);
        f.valid.resize((size_t)neighbourhood(cu.cc, f.valid.data()));
        f.n_last[0] = bs[s]->feat_h[(size_t)scans[s] * 4 + 1]; f.n_last[1] = bs[s]->feat_h[(size_t)scans[s] * 4 + 3];
        if (f.n_last[0] > kMapStackMax || f.n_last[1] > kMapStackMax) { c->err = "lmono_mapper: scan cloud too large"; return LMONO_ECAPACITY; }
    }
    return LMONO_OK;
}
// Round 4: the frame's first half is enqueued in one go -- the host does not wait for the voxel filter's counts before it launches the optimisation
// (the kernels read them from the device, their launches are sized by the clouds' sizes before the filter and stride), it learns them from an event
// while the optimisation runs, enqueues the cube assignment behind the solve, and waits ONCE for poses, statistics and cube indices.  Everything the
// first half needs travels in ONE upload (the frame blob: poses, zeroed statistics and barrier counters, the filter's counts, all job tables).
// ---- phase 3 first, on the side stream (both are chains of short launches that leave most of the chip idle, and neither needs the other): map clouds
// of the neighbourhoods, concatenated in validInd order, and their grids for the streams whose map is large enough
int BatchCall::gather_phase()
{
    side_guard.s = side;
    std::vector<CopyJob> jobs;
    for (int s = 0; s < n; s++) {
        lmono_mapper *m = ms[s];
        FrameState &f = F[(size_t)s];
        for (int t = 0; t < 2; t++) {
            f.n_map[t] = 0;
            for (int ind : f.valid) {
                const Seg &sg = m->cube[(size_t)t][(size_t)ind];
                if (sg.n == 0) continue;
                if (f.n_map[t] + sg.n > kMapNeighMax) { c->err = "lmono_mapper: neighbourhood holds more than 1 Mi points"; return LMONO_ECAPACITY; }
                push_copy(jobs, m->arena[t][m->half[t]] + sg.off, m->neigh[t] + f.n_map[t], sg.n);
                f.n_map[t] += sg.n;
            }
        }
        if (f.n_map[0] > 10 && f.n_map[1] > 50) act.push_back(s);
    }
    // one upload: [CopyJob x jobs | CloudJob x 2 act]
    std::vector<CloudJob> cj((size_t)2 * act.size());
    int max_nmap = 0;
    for (size_t a = 0; a < act.size(); a++) {
        const FrameState &f = F[(size_t)act[a]];
        for (int t = 0; t < 2; t++) {
            cj[2 * a + (size_t)t] = neigh_cloud_job(ms[act[a]], t, f.n_map[t]);
            max_nmap = std::max(max_nmap, f.n_map[t]);
        }
    }
    if (!jobs.empty() || !cj.empty()) {
        const size_t cj_at = al16(jobs.size() * sizeof(CopyJob));
        std::vector<char> &blob = side_blob;          // the call's: alive until every stream has been waited for
        blob.resize(cj_at + cj.size() * sizeof(CloudJob));
        if (!jobs.empty()) memcpy(blob.data(), jobs.data(), jobs.size() * sizeof(CopyJob));
        if (!cj.empty()) memcpy(blob.data() + cj_at, cj.data(), cj.size() * sizeof(CloudJob));
        if (const int rc = js.upload(c, blob.data(), blob.size(), side)) return rc;
        if (!jobs.empty()) hipLaunchKernelGGL(k_copy_jobs, dim3((unsigned)jobs.size()), dim3(256), 0, side, (const CopyJob *)js.last);
        if (!cj.empty()) launch_cloud_grids(side, (const CloudJob *)((const char *)js.last + cj_at), (int)cj.size(), max_nmap);
    }
    HIP_TRY(c, hipEventRecord(m0->ev_side, side));
    return LMONO_OK;
}
// ---- the frame blob: [x 8n doubles | stats 8n | barriers 16n | filter counts 2n | VoxJob 2n | tile table | MapStream act | AssignJob 2n]; behind its
// upload, phase 2 (the scan filter) and phase 4 (the optimisation) on the main stream
int BatchCall::optimise_phase()
{
    int rc;
    if ((rc = pin_grow(c, m0, m0->pin_i, m0->pin_i_cap, (size_t)2 * n)) || (rc = pin_grow(c, m0, m0->pin_x, m0->pin_x_cap, (size_t)12 * n))) return rc;
    ns_h = m0->pin_i; xh = m0->pin_x; stats = (int *)(m0->pin_x + (size_t)8 * n);
    for (size_t k = 0; k < (size_t)8 * n; k++) stats[k] = 0;
    int n_last_total = 0;
    std::vector<VoxJob> vj((size_t)2 * n);
    std::vector<int> tab;
    std::vector<MapStream> S(act.size());
    std::vector<AssignJob> aj((size_t)2 * n);
    for (int s = 0; s < n; s++) n_last_total += F[(size_t)s].n_last[0] + F[(size_t)s].n_last[1];
    if ((rc = mp_grow(c, m0, m0->cubebuf, m0->cubebuf_cap, (size_t)n_last_total + 1))) return rc;
    // sizes first: the tile table needs the jobs' sizes only
    for (int s = 0; s < n; s++) for (int t = 0; t < 2; t++) vj[(size_t)2 * s + t].n = F[(size_t)s].n_last[t];
    vox_tile_table(vj.data(), vj.size(), tab);
    const size_t o_x = 0, o_stats = o_x + sizeof(double) * 8 * (size_t)n, o_bar = o_stats + sizeof(int) * 8 * (size_t)n, o_ns = o_bar + sizeof(int) * 16 * (size_t)n,
                 o_vox = al16(o_ns + sizeof(int) * 2 * (size_t)n), o_tab = al16(o_vox + vj.size() * sizeof(VoxJob)), o_S = al16(o_tab + tab.size() * sizeof(int)),
                 o_aj = al16(o_S + S.size() * sizeof(MapStream)), bytes = o_aj + aj.size() * sizeof(AssignJob);
    if ((rc = js.place(c, bytes))) return rc;
    char *base = (char *)js.last;
    double *xb = (double *)(base + o_x);
    int *statbuf = (int *)(base + o_stats), *nsb = (int *)(base + o_ns);
    unsigned int *barbuf = (unsigned int *)(base + o_bar);
    x_d = xb; aj_d = (const AssignJob *)(base + o_aj);
    for (int s = 0; s < n; s++)
        for (int t = 0; t < 2; t++) {
            lmono_mapper *m = ms[s];
            scan_vox_job(vj[(size_t)2 * s + t], m, bs[s], scans[s], t, m->vk[t], m->vi[t], m->vws[t], nsb + 2 * s + t);
            aj[(size_t)2 * s + t] = { m->stack[t], 0, nsb, 2 * s + t, xb + 8 * s, m->cen[0], m->cen[1], m->cen[2], m->newpts[t], m0->cubebuf };
        }
    int max_nq = 0;        // upper bound: the clouds before the filter
    for (size_t a = 0; a < act.size(); a++) {
        const FrameState &f = F[(size_t)act[a]];
        S[a] = map_stream(ms[act[a]], f.n_map, nsb + 2 * act[a], xb + 8 * act[a], statbuf + 8 * act[a], barbuf + 16 * act[a]);
        max_nq = std::max(max_nq, f.n_last[0] + f.n_last[1]);
    }
    vox_blob.assign(bytes, 0);                                   // statistics, barrier counters and filter counts start at zero
    for (int s = 0; s < n; s++) for (int k = 0; k < 8; k++) ((double *)(vox_blob.data() + o_x))[(size_t)8 * s + k] = F[(size_t)s].x[k];
    memcpy(vox_blob.data() + o_vox, vj.data(), vj.size() * sizeof(VoxJob));
    if (!tab.empty()) memcpy(vox_blob.data() + o_tab, tab.data(), tab.size() * sizeof(int));
    if (!S.empty()) memcpy(vox_blob.data() + o_S, S.data(), S.size() * sizeof(MapStream));
    memcpy(vox_blob.data() + o_aj, aj.data(), aj.size() * sizeof(AssignJob));
    if ((rc = js.send(c, vox_blob.data(), bytes, st))) return rc;
    // ---- phase 2: VoxelGrid of the scan clouds (read in place from the scan batches), on the main stream
    launch_voxel_jobs(st, (const VoxJob *)(base + o_vox), (const int *)(base + o_tab), (int)tab.size(), 4);
    HIP_TRY(c, hipMemcpyAsync(ns_h, nsb, sizeof(int) * 2 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipEventRecord(m0->ev_sizes, st));
    tp[2] = tnow();
    tp[3] = tp[2];
    // ---- phase 4: optimisation (2 x [correspond + solve]) behind both streams, enqueued at once
    HIP_TRY(c, hipStreamWaitEvent(st, m0->ev_side, 0));
    if (!act.empty()) launch_map_optimise(st, (const MapStream *)(base + o_S), (int)act.size(), max_nq, c->map_budget);
    return LMONO_OK;
}
// ---- the filter's counts (the optimisation is running): exact sizes for the assignment and the copies back; then phase 5: pointAssociateToMap + cube
// index of every stack point with the refined pose, behind the solve (its table went up with the blob: sizes and the dense layout of the cube indices
// come from the device-side counts); then the one wait
int BatchCall::assign_phase()
{
    int rc;
    HIP_TRY(c, hipEventSynchronize(m0->ev_sizes));
    for (int s = 0; s < n; s++) { F[(size_t)s].n_stack[0] = ns_h[(size_t)2 * s]; F[(size_t)s].n_stack[1] = ns_h[(size_t)2 * s + 1]; }
    for (int k = 0; k < 2 * n; k++) if (ns_h[k] < 0) { c->err = "lmono_mapper: voxel filter rejected a scan cloud"; return LMONO_ECAPACITY; }
    pos_at.resize((size_t)2 * n);
    for (int s = 0; s < n; s++) for (int t = 0; t < 2; t++) { pos_at[(size_t)2 * s + t] = pos_total; pos_total += (size_t)F[(size_t)s].n_stack[t]; max_ns = std::max(max_ns, F[(size_t)s].n_stack[t]); }
    if ((rc = pin_grow(c, m0, m0->pin_cube, m0->pin_cube_cap, pos_total + 1))) return rc;
    int *cube_all = m0->pin_cube;
    if (max_ns > 0) {
        hipLaunchKernelGGL(k_map_assign, dim3((max_ns + 255) / 256, 2 * n), dim3(256), 0, st, aj_d);
        HIP_TRY(c, hipMemcpyAsync(cube_all, m0->cubebuf, sizeof(int) * pos_total, hipMemcpyDeviceToHost, st));
    }
    if (!act.empty()) HIP_TRY(c, hipMemcpyAsync(xh, x_d, sizeof(double) * 8 * (size_t)n + sizeof(int) * 8 * (size_t)n, hipMemcpyDeviceToHost, st));      // poses + statistics: adjacent in the blob
    HIP_TRY(c, hipStreamSynchronize(st));
    tp[4] = tnow();
    for (int s : act) if (stats[(size_t)s * 8 + 6]) { c->err = "lmono_mapper: a solve's cluster barrier timed out"; return LMONO_ENODEV; }
    for (int s : act) for (int k = 0; k < 8; k++) F[(size_t)s].x[k] = xh[(size_t)8 * s + k];
    for (int s = 0; s < n; s++) for (int t = 0; t < 2; t++) F[(size_t)s].cube_h[t] = cube_all + pos_at[(size_t)2 * s + t];
    return LMONO_OK;
}
// results, transformUpdate (host)
void BatchCall::results_phase()
{
    for (int s = 0; s < n; s++) {
        const FrameState &f = F[(size_t)s];
        for (int k = 0; k < 4; k++) q_w_curr[4 * s + k] = f.x[k];
        for (int k = 0; k < 3; k++) t_w_curr[3 * s + k] = f.x[4 + k];
        if (stats_h) {
            for (int k = 0; k < 6; k++) stats_h[(size_t)s * 8 + k] = stats[(size_t)s * 8 + k];
            stats_h[(size_t)s * 8 + 6] = f.n_map[0] + f.n_map[1];       // map points of the neighbourhood
            stats_h[(size_t)s * 8 + 7] = 0;                             // points of the cubes the update rebuilds: added by the plan
        }
        transform_update(ms[s], f.x, q_wodom + 4 * s, t_wodom + 3 * s);
    }
}
// the update plan of stream s, made by worker thread tid with its own per-cube tables
void BatchCall::plan_stream(int s, int tid)
{
    MapPlanScratch &ps = c->plan_scratch[(size_t)tid];
    std::vector<char> &is_valid = ps.is_valid;
    std::vector<int> &add = ps.add, &fill = ps.fill, &cand = ps.cand;
    std::vector<int64_t> &cat_off = ps.cat_off;
    std::vector<MapPlanScratch::Run> &runs = ps.runs;
    PlanOut &out = outs[(size_t)s];
    lmono_mapper *m = ms[s];
    FrameState &f = F[(size_t)s];
    for (int ind : f.valid) is_valid[(size_t)ind] = 1;
    for (int t = 0; t < 2 && !out.err; t++) {
        // candidates in ascending cube order: the neighbourhood and every other cube a new point falls into
        // (the stack is in voxel order: neighbours in it mostly share a cube -- the per-point work is done per RUN of equal cube indices)
        cand.assign(f.valid.begin(), f.valid.end());
        runs.clear();
        int *ph = pos_all + pos_at[(size_t)2 * s + t];
        {
            const int *ch = f.cube_h[t];
            const int ns = f.n_stack[t];
            for (int i = 0; i < ns;) {
                const int ind = ch[i];
                int e = i + 1;
                while (e < ns && ch[e] == ind) e++;
                if (ind >= 0) {
                    runs.push_back({ ind, i, e - i });
                    if (add[(size_t)ind] == 0 && !is_valid[(size_t)ind]) cand.push_back(ind);
                    add[(size_t)ind] += e - i;
                } else
                    for (int k = i; k < e; k++) ph[k] = -1;        // outside the cube array: not placed
                i = e;
            }
        }
        std::sort(cand.begin(), cand.end());
        int64_t at = 0;
        for (int ind : cand) {
            const Seg &sg = m->cube[(size_t)t][(size_t)ind];
            const bool v = is_valid[(size_t)ind] != 0;
            if (!((v && sg.n + add[(size_t)ind] > 0) || (!v && add[(size_t)ind] > 0))) continue;
            cat_off[(size_t)ind] = at;
            if (sg.n > 0) push_copy(out.copy, m->arena[t][m->half[t]] + sg.off, m->cat[t] + at, sg.n);
            const int n_in = sg.n + add[(size_t)ind];
            if (v && n_in > kVoxCloudMax && !out.err) out.err = "lmono_mapper: a cube holds more than 65536 points";
            out.touched.push_back({ s, t, ind, n_in, at, v });
            at += n_in;
        }
        if (at > (int64_t)kMapNeighMax + kMapStackMax && !out.err) out.err = "lmono_mapper: frame touches more points than the workspace holds";
        if (!out.err)
            for (const MapPlanScratch::Run &r : runs) {
                const int p0 = (int)(cat_off[(size_t)r.ind] + m->cube[(size_t)t][(size_t)r.ind].n + fill[(size_t)r.ind]);
                fill[(size_t)r.ind] += r.len;
                for (int k = 0; k < r.len; k++) ph[r.at + k] = p0 + k;
            }
        for (int ind : cand) { add[(size_t)ind] = 0; fill[(size_t)ind] = 0; cat_off[(size_t)ind] = -1; }
        sj[(size_t)2 * s + t] = { m->newpts[t], nullptr, f.n_stack[t], m->cat[t] };       // .pos: set when the blob is placed
    }
    for (int ind : f.valid) is_valid[(size_t)ind] = 0;
}
// ---- phase 6: the scans join the cubes.  Host: per touched cube [old points | new points in stack order]; device: build
// them, re-filter the cubes of the neighbourhoods into fresh arena space, the other touched cubes keep [old | new]
// (the per-cube tables are allocated once per call and only the entries a stream touched are reset: 64 streams x 2 types x 4851 cubes of
// fresh vectors were a millisecond of host time per batched frame)
int BatchCall::plan_phase()
{
    int rc;
    // the update's tables travel in ONE upload from a pinned staging buffer, the placements first (they are written straight into it):
    // [pos | CopyJob x copy | ScatterJob x 2 n | VoxJob x vox | tile table | CopyJob x keep]; the tables behind the placements are bounded per stream
    o_copy = al16((pos_total + 1) * sizeof(int)); tables_cap = (size_t)n * (96 << 10);
    if ((rc = pin_grow(c, m0, m0->pin_blob, m0->pin_blob_cap, o_copy + tables_cap))) return rc;
    pos_all = (int *)m0->pin_blob;
    sj.resize((size_t)2 * n);
    // The streams are independent: every stream's plan is made by one worker thread into the stream's own lists (touched cubes, copy jobs) and its own
    // range of the placements; the lists are joined in stream order afterwards, so the tables are the ones a single loop over the streams writes.
    // (64 streams on the caller's thread: 0.75 ms of a 3.5-ms batched frame with the GPU idle.)
    if (!c->workers && n >= 8) {
        int nt = 0;
        if (const char *e = getenv("LMONO_LIB_THREADS")) nt = atoi(e);
        if (nt <= 0) nt = (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency()));        // (4 / 8 / 16 threads: plan 0.36 / 0.26 / 0.25 ms for 64 streams)
        c->workers.reset(new HostWorkers(nt));
    }
    const int T = c->workers && n >= 8 ? c->workers->threads() : 1;
    if ((int)c->plan_scratch.size() < T) c->plan_scratch.resize((size_t)T);      // (every stream leaves its thread's tables as it found them: they live from call to call)
    outs.resize((size_t)n);
    bool planned = true;
    if (T > 1) planned = c->workers->run(n, [this](int s, int tid) { plan_stream(s, tid); });
    else { try { for (int s = 0; s < n; s++) plan_stream(s, 0); } catch (...) { planned = false; } }
    if (!planned) { c->plan_scratch.clear(); c->err = "lmono_mapper: out of host memory while planning the map update"; return LMONO_ENOMEM; }      // (the tables may be half-written)
    for (int s = 0; s < n; s++) if (outs[(size_t)s].err) { c->err = outs[(size_t)s].err; return LMONO_ECAPACITY; }
    size_t nt_total = 0, nc_total = 0;
    for (const PlanOut &o : outs) { nt_total += o.touched.size(); nc_total += o.copy.size(); }
    touched.reserve(nt_total); copy.reserve(nc_total);
    for (const PlanOut &o : outs) { touched.insert(touched.end(), o.touched.begin(), o.touched.end()); copy.insert(copy.end(), o.copy.begin(), o.copy.end()); }
    if (stats_h) for (const Touched &T : touched) stats_h[(size_t)T.s * 8 + 7] += T.n_in;
    return LMONO_OK;
}
// arena space (an output is never larger than its input); compaction reads only the tables, `cat` is already built
int BatchCall::arena_phase()
{
    int rc;
    std::vector<int64_t> need((size_t)2 * n, 0);
    for (const Touched &T : touched) need[(size_t)2 * T.s + T.t] += T.n_in;
    for (int s = 0; s < n; s++)
        for (int t = 0; t < 2; t++)
            if (ms[s]->bump[t] + need[(size_t)2 * s + t] > kMapArena) {
                if ((rc = mapper_compact(ms[s], t))) return rc;
                if (ms[s]->bump[t] + need[(size_t)2 * s + t] > kMapArena) { c->err = "lmono_mapper: map arena exhausted"; return LMONO_ECAPACITY; }
            }
    return LMONO_OK;
}
// the update's tables, their ONE upload, its launches, the ONE wait for it and the commit of the new segments to the mappers' tables
int BatchCall::update_phase()
{
    int rc;
    std::vector<size_t> vox_t;
    std::vector<int64_t> new_off(touched.size());
    std::vector<size_t> ws_at((size_t)2 * n, 0);
    int cube_passes = 1;
    for (size_t k = 0; k < touched.size(); k++) {
        const Touched &T = touched[k];
        lmono_mapper *m = ms[T.s];
        float4 *dst = m->arena[T.t][m->half[T.t]] + m->bump[T.t];
        new_off[k] = m->bump[T.t];
        if (T.filter) {
            VoxJob J;
            J.in = m->cat[T.t] + T.cat_off; J.n = T.n_in; J.inv_leaf = 1.0f / m->leaf[T.t]; J.out = dst; J.n_out = nullptr;
            J.key_a = m->vk[T.t] + 2 * T.cat_off; J.key_b = J.key_a + T.n_in; J.idx_a = m->vi[T.t] + 2 * T.cat_off; J.idx_b = J.idx_a + T.n_in;
            size_t &wa = ws_at[(size_t)2 * T.s + T.t];
            if (wa + vox_ws_ints(T.n_in) > m->vws_cap) { c->err = "lmono_mapper: voxel workspace exhausted"; return LMONO_ECAPACITY; }
            J.ws = m->vws[T.t] + wa; wa += vox_ws_ints(T.n_in);
            cube_passes = std::max(cube_passes, cube_filter_passes(m->leaf[T.t]));
            vox.push_back(J); vox_t.push_back(k);
        } else {
            push_copy(keep, m->cat[T.t] + T.cat_off, dst, T.n_in);
        }
        m->bump[T.t] += T.n_in;
    }
    // output sizes of the filter jobs land in one array owned by the first mapper (grown on demand)
    if ((rc = pin_grow(c, m0, m0->pin_nout, m0->pin_nout_cap, vox.size() + 1))) return rc;
    int *nout_h = m0->pin_nout;
    if ((rc = mp_grow(c, m0, m0->nout_big, m0->nout_cap, vox.size()))) return rc;
    for (size_t k = 0; k < vox.size(); k++) vox[k].n_out = m0->nout_big + k;
    // ONE upload for the whole update (layout in batch_plan_phase)
    {
        std::vector<int> tab;
        vox_tile_table(vox.data(), vox.size(), tab);
        const size_t o_pos = 0, o_sj = al16(o_copy + copy.size() * sizeof(CopyJob)), o_vox = al16(o_sj + sj.size() * sizeof(ScatterJob)),
                     o_tab = al16(o_vox + vox.size() * sizeof(VoxJob)), o_keep = al16(o_tab + tab.size() * sizeof(int)), bytes = o_keep + keep.size() * sizeof(CopyJob);
        if (bytes > o_copy + tables_cap) { c->err = "lmono_mapper: the update's job tables exceed their staging bound"; return LMONO_ECAPACITY; }
        if ((rc = js.place(c, bytes))) return rc;
        const char *base = (const char *)js.last;
        for (int s = 0; s < n; s++) for (int t = 0; t < 2; t++) sj[(size_t)2 * s + t].pos = (const int *)(base + o_pos) + pos_at[(size_t)2 * s + t];
        char *stage = m0->pin_blob;
        if (!copy.empty()) memcpy(stage + o_copy, copy.data(), copy.size() * sizeof(CopyJob));
        memcpy(stage + o_sj, sj.data(), sj.size() * sizeof(ScatterJob));
        if (!vox.empty()) memcpy(stage + o_vox, vox.data(), vox.size() * sizeof(VoxJob));
        if (!tab.empty()) memcpy(stage + o_tab, tab.data(), tab.size() * sizeof(int));
        if (!keep.empty()) memcpy(stage + o_keep, keep.data(), keep.size() * sizeof(CopyJob));
        if ((rc = js.send(c, stage, bytes, st))) return rc;
        if (!copy.empty()) hipLaunchKernelGGL(k_copy_jobs, dim3((unsigned)copy.size()), dim3(256), 0, st, (const CopyJob *)(base + o_copy));
        if (max_ns > 0) hipLaunchKernelGGL(k_scatter_pos, dim3((max_ns + 255) / 256, 2 * n), dim3(256), 0, st, (const ScatterJob *)(base + o_sj));
        if (!vox.empty()) {
            launch_voxel_jobs(st, (const VoxJob *)(base + o_vox), (const int *)(base + o_tab), (int)tab.size(), cube_passes);
            HIP_TRY(c, hipMemcpyAsync(nout_h, m0->nout_big, sizeof(int) * vox.size(), hipMemcpyDeviceToHost, st));
        }
        if (!keep.empty()) hipLaunchKernelGGL(k_copy_jobs, dim3((unsigned)keep.size()), dim3(256), 0, st, (const CopyJob *)(base + o_keep));
    }
    tpb = tnow();
    HIP_TRY(c, hipStreamSynchronize(st));       // ONE wait for the frame's map update: filter sizes are back, `cat` and the job tables are free
    for (size_t k = 0; k < touched.size(); k++) {
        const Touched &T = touched[k];
        Seg &sg = ms[T.s]->cube[(size_t)T.t][(size_t)T.ind];
        sg.off = new_off[k]; sg.n = T.n_in;
    }
    for (size_t v = 0; v < vox.size(); v++) {
        if (nout_h[v] < 0) { c->err = "lmono_mapper: voxel filter rejected a cube"; return LMONO_ECAPACITY; }
        const Touched &T = touched[vox_t[v]];
        ms[T.s]->cube[(size_t)T.t][(size_t)T.ind].n = nout_h[v];
    }
    tp[6] = tnow();
    return check_launch(c, "mapper kernels");
}
}

extern "C" int lmono_mapper_process_batch(lmono_ctx *c, int n, lmono_mapper *const *ms, lmono_scan_batch *const *bs, const int *scans,
                                          const double *q_wodom, const double *t_wodom, double *q_w_curr, double *t_w_curr, int32_t *stats_h)
{
    if (!c || n <= 0 || !ms || !bs || !scans || !q_wodom || !t_wodom || !q_w_curr || !t_w_curr) return LMONO_EINVAL;
    for (int s = 0; s < n; s++) {
        if (!ms[s] || !bs[s] || !bs[s]->registered || scans[s] < 0 || scans[s] >= bs[s]->n_scans) return LMONO_EINVAL;
        for (int u = 0; u < s; u++) if (ms[u] == ms[s]) { c->err = "lmono_mapper_process_batch: a mapper appears twice"; return LMONO_EINVAL; }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    for (int s = 0; s < n; s++) { const int rcv = mapper_tables_to_host(c, ms[s]); if (rcv) return rcv; }
    BatchCall B{ c, n, ms, bs, scans, q_wodom, t_wodom, q_w_curr, t_w_curr, stats_h, ms[0], c->stream, ms[0]->side, JobScratch{ ms[0] } };
    HIP_TRY(c, hipStreamSynchronize(B.st));        // the previous frame's kernels are done with the job scratch (normally a no-op: a frame ends with a read-back)
    B.F.resize((size_t)n); B.undo.u.reserve((size_t)n);
    for (int s = 0; s < n; s++) B.undo.u.emplace_back(ms[s]);
    int rc;
    B.tp[0] = tnow();
    if ((rc = B.host_phase())) return rc;
    B.tp[1] = tnow();
    if ((rc = B.gather_phase()) || (rc = B.optimise_phase()) || (rc = B.assign_phase())) return rc;
    B.results_phase();
    B.tp[5] = tnow();
    if ((rc = B.plan_phase())) return rc;
    B.tpa = tnow();
    if ((rc = B.arena_phase()) || (rc = B.update_phase())) return rc;
    B.undo.committed = true;
    if (getenv("LMONO_MAP_PROF")) {
        const double *tp = B.tp;
        fprintf(stderr, "MAPPROF n=%d ms: host1 %.2f voxel %.2f gather %.2f optimise %.2f assign %.2f update %.2f (plan %.2f tables+launch %.2f wait %.2f)\n", n, tp[1] - tp[0], tp[2] - tp[1], tp[3] - tp[2], tp[4] - tp[3], tp[5] - tp[4], tp[6] - tp[5], B.tpa - tp[5], B.tpb - B.tpa, tp[6] - B.tpb);
        int mx = 0, n_small = 0; long sum = 0;
        for (const VoxJob &J : B.vox) { mx = std::max(mx, J.n); sum += J.n; n_small += J.n <= 2048; }
        fprintf(stderr, "MAPSIZES scan %d %d -> %d %d  map %d %d  cube jobs %zu (<= 2048: %d) max %d sum %ld kept %zu\n", B.F[0].n_last[0], B.F[0].n_last[1], B.F[0].n_stack[0], B.F[0].n_stack[1],
                B.F[0].n_map[0], B.F[0].n_map[1], B.vox.size(), n_small, mx, sum, B.keep.size());
    }
    return LMONO_OK;
}

extern "C" int lmono_mapper_process(lmono_ctx *c, lmono_mapper *m, lmono_scan_batch *b, int scan, const double q_wodom[4], const double t_wodom[3],
                                    double q_w_curr[4], double t_w_curr[3], int32_t *stats_h)
{
    if (!c || !m || !b || !q_wodom || !t_wodom || !q_w_curr || !t_w_curr) return LMONO_EINVAL;
    if (!b->registered || scan < 0 || scan >= b->n_scans) return LMONO_EINVAL;
    static const bool host_tables = getenv("LMONO_MAP_HOST_TABLES") != nullptr;       // measurement switch: the round-4 frame (cube table on the host, two waits)
    if (host_tables) return lmono_mapper_process_batch(c, 1, &m, &b, &scan, q_wodom, t_wodom, q_w_curr, t_w_curr, stats_h);
    return mapper_process_dev(c, m, b, scan, q_wodom, t_wodom, q_w_curr, t_w_curr, stats_h);
}

extern "C" int lmono_mapper_cube(lmono_ctx *c, lmono_mapper *m, int which, int i, int j, int k, float *out_h, int cap)
{
    if (!c || !m || which < 0 || which > 1 || i < 0 || i >= kMapW || j < 0 || j >= kMapH || k < 0 || k >= kMapD) return LMONO_EINVAL;
    Seg s = m->cube[(size_t)which][(size_t)(i + kMapW * j + kMapW * kMapH * k)];
    if (m->dev_mode) {          // the table is on the device: behind the last frame's map update
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        int2 e;
        HIP_TRY(c, hipMemcpy(&e, &m->dev->tab[which][i + kMapW * j + kMapW * kMapH * k], sizeof(e), hipMemcpyDeviceToHost));
        s.off = e.x; s.n = e.y;
    }
    if (!out_h) return s.n;
    if (s.n > cap) return LMONO_ECAPACITY;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (s.n > 0) HIP_TRY(c, hipMemcpy(out_h, m->arena[which][m->half[which]] + s.off, sizeof(float) * 4 * (size_t)s.n, hipMemcpyDeviceToHost));
    return s.n;
}
