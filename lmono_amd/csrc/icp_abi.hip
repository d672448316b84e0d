// icp_abi.hip -- C ABI of the point-to-point ICP (included by lmono_hip.hip after sor_abi.hip: align_frames reads a map builder, align_filtered an
// outlier filter, set_target_map a voxel map, and insert_aligned feeds a voxel map)
#pragma once
#include "icp.hip"

struct lmono_icp {
    lmono_ctx *ctx = nullptr;
    int64_t max_src = 0, max_tgt = 0;
    float D = 0.0f, D2 = 0.0f;
    int max_iter = 0, poll = 2;                  // poll: pairs of launches between two reads of the done words
    double eps = 0.0, mse_eps = 0.0;
    double G[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    DevOwner mem;
    // the target: its grid (with an origin); tpts: staging of the host-buffer and the voxel-map entries, n_vox: the points the latter wrote
    CellGrid grid;
    PtRgb *tpts = nullptr;
    unsigned *n_vox = nullptr;
    bool has_target = false;
    int64_t tn = 0, t_rejected = 0;
    float o[3] = { 0.0f, 0.0f, 0.0f };
    // the source and the last align
    PtRgb *spts = nullptr, *out = nullptr;       // spts: staging of the host-buffer entry
    IcpU *u = nullptr;
    float *d2 = nullptr;
    IcpDev *dev = nullptr;
    long long *hist = nullptr;
    bool aligned = false;
    int64_t last_n = 0, stats[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    IcpState last;
    double last_G[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    float last_o[3] = { 0.0f, 0.0f, 0.0f };
    // per-call job table + done words of a batch led by this aligner
    IcpJob *jobs = nullptr;
    int *results = nullptr;
    int jobs_cap = 0;
};

static constexpr int64_t kIcpMaxPoints = (int64_t)1 << 28;

extern "C" void lmono_icp_destroy(lmono_icp *s) { delete s; }

extern "C" float lmono_icp_default_cell(float max_corr) { return icp_default_cell(max_corr); }

extern "C" lmono_icp *lmono_icp_create(lmono_ctx *c, int64_t max_source_points, int64_t max_target_points, float max_corr, int max_iter, double eps, double mse_eps,
                                       float cell, int max_rings)
{
    if (!c) return nullptr;
    if (max_source_points < 1 || max_source_points > kIcpMaxPoints || max_target_points < 1 || max_target_points > kIcpMaxPoints ||
        !icp_params_ok(max_corr, max_iter, eps, mse_eps, cell, max_rings)) {
        c->err = "lmono_icp_create: point counts in 1 .. 2^28, 0 < max_corr <= 16, max_iter in 1 .. 65536, eps >= 0, mse_eps >= 0, cell > 0 (with a finite 1 / cell), "
                 "max_rings in 1 .. 64, (max_rings - 0.25) cell >= max_corr";
        return nullptr;
    }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return nullptr; }
    lmono_icp *s = new lmono_icp();
    s->ctx = c;
    s->max_src = max_source_points; s->max_tgt = max_target_points;
    s->D = max_corr; s->D2 = max_corr * max_corr; s->max_iter = max_iter; s->eps = eps; s->mse_eps = mse_eps;
    icp_state_init(s->last);
    const size_t ns = (size_t)max_source_points, nt = (size_t)max_target_points;
    const bool ok = s->grid.alloc(s->mem, max_target_points, cell, max_rings, /*work_list=*/false) && s->mem.alloc_zero(s->n_vox, 1) && s->mem.alloc(s->tpts, nt) &&
                    s->mem.alloc(s->spts, ns) && s->mem.alloc(s->out, ns) && s->mem.alloc(s->u, ns) && s->mem.alloc(s->d2, ns) && s->mem.alloc_zero(s->dev, 1) && s->mem.alloc(s->hist, 2 * (size_t)max_iter);
    if (!ok) { c->err = "lmono_icp_create: device allocation failed"; lmono_icp_destroy(s); return nullptr; }
    return s;
}

extern "C" int lmono_icp_set_guess(lmono_ctx *c, lmono_icp *s, const double *g)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    static const double ident[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    if (g) for (int k = 0; k < 12; k++) if (!std::isfinite(g[k])) { c->err = "lmono_icp_set_guess: non-finite entry"; return LMONO_EINVAL; }
    std::memcpy(s->G, g ? g : ident, sizeof s->G);
    return LMONO_OK;
}

extern "C" int lmono_icp_set_poll_interval(lmono_ctx *c, lmono_icp *s, int pairs)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    if (pairs < 1) { c->err = "lmono_icp_set_poll_interval: at least 1"; return LMONO_EINVAL; }
    s->poll = pairs;
    return LMONO_OK;
}

// the job of one stream; the source half is filled by the align
static void icp_job_target(const lmono_icp *s, IcpJob &j)
{
    j.g = s->grid.view(nullptr, s->tn);
    j.D2 = s->D2;
    j.pts = nullptr; j.n = 0; j.u = s->u; j.d2 = s->d2; j.out = s->out; j.dev = s->dev; j.hist = s->hist; j.done = nullptr;
    j.max_iter = s->max_iter; j.eps = s->eps; j.mse_eps = s->mse_eps;
    std::memcpy(j.G, s->G, sizeof j.G);
}

// the target of s from n points in device memory (n <= max_tgt): five launches (one for n == 0), one read-back; ends synchronised
static int icp_build_target(lmono_ctx *c, const char *who, lmono_icp *s, const PtRgb *pts_d, int64_t n)
{
    s->has_target = false;
    if (!job_table(s->mem, s->jobs, s->results, s->jobs_cap, 1, 1)) { c->err = std::string(who) + ": job table allocation failed"; return LMONO_ENOMEM; }
    s->tn = n;
    IcpJob j;
    icp_job_target(s, j);
    j.g.pts = pts_d;
    HIP_TRY(c, hipMemcpyAsync(s->jobs, &j, sizeof j, hipMemcpyHostToDevice, c->stream));
    if (int rc = cellgrid_build</*kOrigin=*/true>(c, s->jobs, 1, n)) return rc;
    CellWords t;
    HIP_TRY(c, hipMemcpyAsync(&t, s->grid.words, sizeof t, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((int64_t)t.alloc + (int64_t)t.rejected != n) { c->err = std::string(who) + ": the target's placed and rejected points do not add up to its size"; return LMONO_ENODEV; }
    for (int a = 0; a < 3; a++) s->o[a] = t.o[a];
    s->t_rejected = t.rejected;
    s->has_target = true;
    return LMONO_OK;
}

extern "C" int lmono_icp_set_target_d(lmono_ctx *c, lmono_icp *s, const lmono_point_rgb *pts_d, int64_t n)
{
    if (!c || !s || s->ctx != c || n < 0 || (n > 0 && !pts_d)) return LMONO_EINVAL;
    if (n > s->max_tgt) { c->err = "lmono_icp_set_target_d: more points than the aligner's max_target_points"; return LMONO_ECAPACITY; }
    return icp_build_target(c, "lmono_icp_set_target_d", s, (const PtRgb *)pts_d, n);
}

extern "C" int lmono_icp_set_target(lmono_ctx *c, lmono_icp *s, const lmono_point_rgb *pts_h, int64_t n)
{
    if (!c || !s || s->ctx != c || n < 0 || (n > 0 && !pts_h)) return LMONO_EINVAL;
    if (n > s->max_tgt) { c->err = "lmono_icp_set_target: more points than the aligner's max_target_points"; return LMONO_ECAPACITY; }
    if (n > 0) HIP_TRY(c, hipMemcpyAsync(s->tpts, pts_h, sizeof(PtRgb) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    const int rc = icp_build_target(c, "lmono_icp_set_target", s, s->tpts, n);
    if (rc != LMONO_OK) (void)hipStreamSynchronize(c->stream);      // an early return must not leave the copy from the caller's buffer in flight
    return rc;
}

extern "C" int lmono_icp_set_target_map(lmono_ctx *c, lmono_icp *s, lmono_voxel_map *m)
{
    if (!c || !s || s->ctx != c || !m || m->ctx != c) return LMONO_EINVAL;
    if (m->n_vox > s->max_tgt) { c->err = "lmono_icp_set_target_map: more voxels than the aligner's max_target_points"; return LMONO_ECAPACITY; }
    if (int rc = m->n_vox > 0 ? vm_enqueue_points(c, m, s->tpts, s->n_vox) : LMONO_OK) return rc;
    if (int rc = icp_build_target(c, "lmono_icp_set_target_map", s, s->tpts, m->n_vox)) return rc;
    if (m->n_vox > 0) {
        unsigned found = 0;
        HIP_TRY(c, hipMemcpy(&found, s->n_vox, sizeof found, hipMemcpyDeviceToHost));
        if ((int64_t)found != m->n_vox) { s->has_target = false; c->err = "lmono_icp_set_target_map: the table's occupied records do not match the map's size"; return LMONO_ENODEV; }
    }
    return LMONO_OK;
}

extern "C" int lmono_icp_set_target_aligned(lmono_ctx *c, lmono_icp *s)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    if (!s->aligned) { c->err = "lmono_icp_set_target_aligned: no align has run"; return LMONO_EINVAL; }
    if (s->last_n > s->max_tgt) { c->err = "lmono_icp_set_target_aligned: more points than the aligner's max_target_points"; return LMONO_ECAPACITY; }
    return icp_build_target(c, "lmono_icp_set_target_aligned", s, s->out, s->last_n);
}

// one align for n aligners: pts_d[s] device clouds of ns[s] points.  One launch per phase for all streams; ends synchronised.
static int icp_align_batch(lmono_ctx *c, const char *who, int n, lmono_icp *const *icps, const PtRgb *const *pts_d, const int64_t *ns, int64_t *stats)
{
    int64_t max_n = 0;
    int max_iter = 0;
    for (int s = 0; s < n; s++) {
        if (!icps[s]->has_target) { c->err = std::string(who) + ": no target has been set"; return LMONO_EINVAL; }
        if (ns[s] > icps[s]->max_src) { c->err = std::string(who) + ": more points than the aligner's max_source_points"; return LMONO_ECAPACITY; }
        max_n = std::max(max_n, ns[s]);
        if (ns[s] > 0) max_iter = std::max(max_iter, icps[s]->max_iter);
    }
    // the handles show an align only once it has ended well: a call that fails on its way leaves them without one (no cloud, no distances, nothing to insert)
    for (int s = 0; s < n; s++) {
        lmono_icp *f = icps[s];
        f->aligned = false; f->last_n = 0;
        icp_state_init(f->last);
        std::memcpy(f->last_G, f->G, sizeof f->G);
        std::memcpy(f->last_o, f->o, sizeof f->o);
        for (int w = 0; w < 8; w++) f->stats[w] = 0;
        f->stats[0] = ns[s]; f->stats[2] = f->tn; f->stats[3] = f->t_rejected; f->stats[5] = f->last.status;
    }
    auto finish = [&] {
        for (int s = 0; s < n; s++) {
            icps[s]->aligned = true; icps[s]->last_n = ns[s];
            if (stats) std::memcpy(stats + 8 * s, icps[s]->stats, sizeof icps[s]->stats);
        }
        return LMONO_OK;
    };
    if (max_n == 0) return finish();                            // nothing to do: no launch
    lmono_icp *lead = icps[0];
    if (!job_table(lead->mem, lead->jobs, lead->results, lead->jobs_cap, n, 1)) { c->err = std::string(who) + ": job table allocation failed"; return LMONO_ENOMEM; }
    std::vector<IcpJob> jobs((size_t)n);
    std::vector<IcpDev> init((size_t)n), fin((size_t)n);
    std::vector<int> done((size_t)n);
    for (int s = 0; s < n; s++) {
        lmono_icp *f = icps[s];
        IcpJob &j = jobs[(size_t)s];
        icp_job_target(f, j);
        j.pts = pts_d[s]; j.n = ns[s]; j.done = lead->results + s;
        std::memset(&init[(size_t)s], 0, sizeof(IcpDev));
        icp_state_init(init[(size_t)s].st);
        done[(size_t)s] = init[(size_t)s].st.done = ns[s] == 0 ? 1 : 0;      // an empty stream runs no iteration, as in a call of its own
        HIP_TRY(c, hipMemcpyAsync(f->dev, &init[(size_t)s], sizeof(IcpDev), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(lead->jobs, jobs.data(), sizeof(IcpJob) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(lead->results, done.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    const dim3 g_pts((unsigned)((max_n + kIcpT - 1) / kIcpT), (unsigned)n), g_one(1, (unsigned)n);
    k_icp_prepare<<<g_pts, kIcpT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_icp_prepare")) return rc;
    for (int it = 1; it <= max_iter; it++) {
        k_icp_step<<<g_pts, kIcpT, 0, c->stream>>>(lead->jobs);
        if (int rc = check_launch(c, "k_icp_step")) return rc;
        k_icp_solve<<<g_one, 64, 0, c->stream>>>(lead->jobs);
        if (int rc = check_launch(c, "k_icp_solve")) return rc;
        if (it % lead->poll == 0 && it < max_iter) {
            HIP_TRY(c, hipMemcpyAsync(done.data(), lead->results, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            bool all = true;
            for (int s = 0; s < n; s++) all = all && done[(size_t)s] != 0;
            if (all) break;
        }
    }
    k_icp_apply<<<g_pts, kIcpT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_icp_apply")) return rc;
    for (int s = 0; s < n; s++) HIP_TRY(c, hipMemcpyAsync(&fin[(size_t)s], icps[s]->dev, sizeof(IcpDev), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int s = 0; s < n; s++) {
        lmono_icp *f = icps[s];
        if (ns[s] == 0) continue;
        const IcpDev &d = fin[(size_t)s];
        if (!d.st.done) { c->err = std::string(who) + ": a stream did not end within max_iter iterations"; return LMONO_ENODEV; }
        f->last = d.st;
        f->stats[1] = (int64_t)d.unusable; f->stats[4] = d.st.k; f->stats[5] = d.st.status; f->stats[6] = d.st.last_n; f->stats[7] = d.st.last_e;
    }
    return finish();
}

extern "C" int lmono_icp_align_d(lmono_ctx *c, lmono_icp *s, const lmono_point_rgb *pts_d, int64_t n, int64_t *stats)
{
    if (!c || !s || s->ctx != c || n < 0 || (n > 0 && !pts_d)) return LMONO_EINVAL;
    const PtRgb *p = (const PtRgb *)pts_d;
    return icp_align_batch(c, "lmono_icp_align_d", 1, &s, &p, &n, stats);
}

extern "C" int lmono_icp_align(lmono_ctx *c, lmono_icp *s, const lmono_point_rgb *pts_h, int64_t n, int64_t *stats)
{
    if (!c || !s || s->ctx != c || n < 0 || (n > 0 && !pts_h)) return LMONO_EINVAL;
    if (n > 0 && n <= s->max_src && s->has_target) HIP_TRY(c, hipMemcpyAsync(s->spts, pts_h, sizeof(PtRgb) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    const PtRgb *p = s->spts;
    const int rc = icp_align_batch(c, "lmono_icp_align", 1, &s, &p, &n, stats);
    if (rc != LMONO_OK) (void)hipStreamSynchronize(c->stream);      // an early return must not leave the copy from the caller's buffer in flight
    return rc;
}

extern "C" int lmono_icp_align_frames(lmono_ctx *c, int n, lmono_icp *const *icps, lmono_map_builder *const *mbs, int64_t *stats)
{
    if (!c || n <= 0 || !icps || !mbs) return LMONO_EINVAL;
    std::vector<const PtRgb *> pts((size_t)n);
    std::vector<int64_t> ns((size_t)n);
    for (int s = 0; s < n; s++) {
        if (!batch_pair_ok(c, "lmono_icp_align_frames", "aligners and map builders", s, icps, mbs)) return LMONO_EINVAL;
        if (!builder_last_cloud(c, "lmono_icp_align_frames", mbs[s], pts[(size_t)s], ns[(size_t)s])) return LMONO_EINVAL;
    }
    return icp_align_batch(c, "lmono_icp_align_frames", n, icps, pts.data(), ns.data(), stats);
}

extern "C" int lmono_icp_align_filtered(lmono_ctx *c, int n, lmono_icp *const *icps, lmono_sor *const *sors, int64_t *stats)
{
    if (!c || n <= 0 || !icps || !sors) return LMONO_EINVAL;
    std::vector<const PtRgb *> pts((size_t)n);
    std::vector<int64_t> ns((size_t)n);
    for (int s = 0; s < n; s++) {
        if (!batch_pair_ok(c, "lmono_icp_align_filtered", "aligners and filters", s, icps, sors)) return LMONO_EINVAL;
        pts[(size_t)s] = sors[s]->out;
        ns[(size_t)s] = sors[s]->last_kept;
    }
    return icp_align_batch(c, "lmono_icp_align_filtered", n, icps, pts.data(), ns.data(), stats);
}

extern "C" int lmono_icp_transform(lmono_ctx *c, lmono_icp *s, double *out)
{
    if (!c || !s || s->ctx != c || !out) return LMONO_EINVAL;
    if (!s->aligned) { c->err = "lmono_icp_transform: no align has run"; return LMONO_EINVAL; }
    icp_transform(s->last, s->last_o, s->last_G, out);
    return LMONO_OK;
}

extern "C" int64_t lmono_icp_cloud(lmono_ctx *c, lmono_icp *s, lmono_point_rgb *out_h, int64_t cap)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    if (!out_h) return s->last_n;
    return read_last(c, "lmono_icp_cloud", s->last_n, cap, out_h, s->out, sizeof(PtRgb));
}

extern "C" int64_t lmono_icp_history(lmono_ctx *c, lmono_icp *s, int64_t *n_e_h, int64_t cap)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    const int64_t k = s->last.k;
    if (!n_e_h) return k;
    return read_last(c, "lmono_icp_history", k, cap, n_e_h, s->hist, 2 * sizeof(int64_t));
}

extern "C" int64_t lmono_icp_distances(lmono_ctx *c, lmono_icp *s, float *d2_h, int64_t cap)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    if (!d2_h) return s->last_n;
    return read_last(c, "lmono_icp_distances", s->last_n, cap, d2_h, s->d2, sizeof(float));
}

extern "C" int lmono_voxel_map_insert_aligned(lmono_ctx *c, int n, lmono_voxel_map *const *maps, lmono_icp *const *icps, int64_t *stats)
{
    if (!c || n <= 0 || !maps || !icps) return LMONO_EINVAL;
    std::vector<const PtRgb *> pts((size_t)n);
    std::vector<int64_t> ns((size_t)n);
    for (int s = 0; s < n; s++) {
        if (!batch_pair_ok(c, "lmono_voxel_map_insert_aligned", "maps and aligners", s, maps, icps)) return LMONO_EINVAL;
        pts[(size_t)s] = icps[s]->out;
        ns[(size_t)s] = icps[s]->last_n;
    }
    return vm_insert_batch(c, "lmono_voxel_map_insert_aligned", n, maps, pts.data(), ns.data(), stats);
}
