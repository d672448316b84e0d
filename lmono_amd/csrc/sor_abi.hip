// sor_abi.hip -- C ABI of the statistical outlier removal (included by lmono_hip.hip after voxel_map_abi.hip: filter_frames reads a map
// builder, insert_filtered feeds a voxel map)
#pragma once
#include "sor.hip"

struct lmono_sor {
    lmono_ctx *ctx = nullptr;
    int64_t max_points = 0;
    int k = 0;
    double mul = 0.0;
    DevOwner mem;
    CellGrid grid;                           // with the query's work list; its words lie in the call's results
    unsigned *v = nullptr, *tile_n = nullptr;
    unsigned char *keep = nullptr;
    PtRgb *out = nullptr, *pts = nullptr;    // pts: staging of the host-buffer entry
    // the last call: points in, kept, and its statistics as the ABI reports them (+ the two diagnostic words)
    int64_t last_n = 0, last_kept = 0, stats[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, diag[2] = { 0, 0 };
    // per-call job table + results of a batch led by this filter
    SorJob *jobs = nullptr;
    int *results = nullptr;
    int jobs_cap = 0;
};

static constexpr int64_t kSorMaxPoints = (int64_t)1 << 28;

extern "C" void lmono_sor_destroy(lmono_sor *s) { delete s; }

extern "C" lmono_sor *lmono_sor_create(lmono_ctx *c, int64_t max_points, int mean_k, double stddev_mul, float cell, int max_rings)
{
    if (!c) return nullptr;
    const bool cell_ok = std::isfinite(cell) && cell > 0.0f && std::isfinite(1.0f / cell) && 1.0f / cell > 0.0f;
    if (max_points < 1 || max_points > kSorMaxPoints || mean_k < 1 || mean_k > kSorMaxK || !std::isfinite(stddev_mul) || !cell_ok || max_rings < 1 ||
        max_rings > kSorMaxRings || !(sor_rho(max_rings, cell) <= kSorMaxRho)) {
        c->err = "lmono_sor_create: max_points in 1 .. 2^28, mean_k in 1 .. 128, stddev_mul finite, cell finite and > 0 (with a finite 1 / cell), max_rings in 1 .. 64, (max_rings - 0.25) cell <= 256";
        return nullptr;
    }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return nullptr; }
    lmono_sor *s = new lmono_sor();
    s->ctx = c;
    s->max_points = max_points; s->k = mean_k; s->mul = stddev_mul;
    const size_t n = (size_t)max_points;
    const bool ok = s->grid.alloc(s->mem, max_points, cell, max_rings, /*work_list=*/true) && s->mem.alloc(s->v, n) && s->mem.alloc(s->tile_n, (n + kSorKeepTile - 1) / kSorKeepTile) &&
                    s->mem.alloc(s->keep, n) && s->mem.alloc(s->out, n) && s->mem.alloc(s->pts, n);
    if (!ok) { c->err = "lmono_sor_create: device allocation failed"; lmono_sor_destroy(s); return nullptr; }
    return s;
}

// one filter call for n filters: pts_d[s] device clouds of ns[s] points.  Seven launches in all, one read-back; ends synchronised.
static int sor_filter_batch(lmono_ctx *c, const char *who, int n, lmono_sor *const *sors, const PtRgb *const *pts_d, const int64_t *ns, int64_t *stats)
{
    int64_t max_n = 0;
    for (int s = 0; s < n; s++) {
        if (ns[s] > sors[s]->max_points) { c->err = std::string(who) + ": more points than the filter's max_points"; return LMONO_ECAPACITY; }
        max_n = std::max(max_n, ns[s]);
    }
    for (int s = 0; s < n; s++) {
        lmono_sor *f = sors[s];
        f->last_n = ns[s]; f->last_kept = 0; f->diag[0] = f->diag[1] = 0;
        for (int w = 0; w < 8; w++) f->stats[w] = 0;
        f->stats[0] = ns[s];
        if (stats) std::memcpy(stats + 8 * s, f->stats, sizeof f->stats);
    }
    if (max_n == 0) return LMONO_OK;                            // nothing to do: no launch
    lmono_sor *lead = sors[0];
    if (!job_table(lead->mem, lead->jobs, lead->results, lead->jobs_cap, n, 2 * kSorWords)) { c->err = std::string(who) + ": job table allocation failed"; return LMONO_ENOMEM; }
    unsigned long long *st = (unsigned long long *)lead->results;
    std::vector<SorJob> jobs((size_t)n);
    for (int s = 0; s < n; s++) {
        lmono_sor *f = sors[s];
        SorJob &j = jobs[(size_t)s];
        j.g = f->grid.view(pts_d[s], ns[s]);
        j.k = f->k; j.mul = f->mul;
        j.v = f->v; j.keep = f->keep; j.tile_n = f->tile_n; j.out = f->out;
        j.st = st + (size_t)kSorWords * s;
        j.g.w = (CellWords *)(j.st + kSorGrid);                 // they come back with the results, in the call's one copy
    }
    HIP_TRY(c, hipMemcpyAsync(lead->jobs, jobs.data(), sizeof(SorJob) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(st, 0, sizeof(unsigned long long) * kSorWords * (size_t)n, c->stream));
    const dim3 g_query((unsigned)std::min<int64_t>(max_n + max_n / kSorQ + 1, 4096), (unsigned)n), g_keep((unsigned)((max_n + kSorKeepTile - 1) / kSorKeepTile), (unsigned)n);
    if (int rc = cellgrid_build</*kOrigin=*/false>(c, lead->jobs, n, max_n)) return rc;
    k_sor_query<<<g_query, kSorQ, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_sor_query")) return rc;
    k_sor_flag<<<g_keep, kSorT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_sor_flag")) return rc;
    k_sor_compact<<<g_keep, kSorT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_sor_compact")) return rc;
    std::vector<unsigned long long> res((size_t)n * kSorWords);
    HIP_TRY(c, hipMemcpyAsync(res.data(), st, sizeof(unsigned long long) * res.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int s = 0; s < n; s++) {
        lmono_sor *f = sors[s];
        if (ns[s] == 0) continue;
        const unsigned long long *r = res.data() + (size_t)kSorWords * s;
        f->stats[1] = (int64_t)((const CellWords *)(r + kSorGrid))->rejected; f->stats[2] = (int64_t)r[kSorIsolated]; f->stats[3] = (int64_t)r[kSorM]; f->stats[4] = (int64_t)r[kSorKept];
        f->stats[5] = (int64_t)r[kSorA]; f->stats[6] = (int64_t)r[kSorBhi]; f->stats[7] = (int64_t)r[kSorBlo];
        f->diag[0] = (int64_t)r[kSorRingSum]; f->diag[1] = (int64_t)r[kSorSelected];
        f->last_kept = f->stats[4];
        if (stats) std::memcpy(stats + 8 * s, f->stats, sizeof f->stats);
    }
    return LMONO_OK;
}

extern "C" int lmono_sor_filter_d(lmono_ctx *c, lmono_sor *s, const lmono_point_rgb *pts_d, int64_t n, int64_t *stats)
{
    if (!c || !s || s->ctx != c || n < 0 || (n > 0 && !pts_d)) return LMONO_EINVAL;
    const PtRgb *p = (const PtRgb *)pts_d;
    return sor_filter_batch(c, "lmono_sor_filter_d", 1, &s, &p, &n, stats);
}

extern "C" int lmono_sor_filter(lmono_ctx *c, lmono_sor *s, const lmono_point_rgb *pts_h, int64_t n, int64_t *stats)
{
    if (!c || !s || s->ctx != c || n < 0 || (n > 0 && !pts_h)) return LMONO_EINVAL;
    if (n > 0 && n <= s->max_points) HIP_TRY(c, hipMemcpyAsync(s->pts, pts_h, sizeof(PtRgb) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    const PtRgb *p = s->pts;
    const int rc = sor_filter_batch(c, "lmono_sor_filter", 1, &s, &p, &n, stats);
    if (rc != LMONO_OK) (void)hipStreamSynchronize(c->stream);      // an early return must not leave the copy from the caller's buffer in flight
    return rc;
}

extern "C" int lmono_sor_filter_frames(lmono_ctx *c, int n, lmono_sor *const *sors, lmono_map_builder *const *mbs, int64_t *stats)
{
    if (!c || n <= 0 || !sors || !mbs) return LMONO_EINVAL;
    std::vector<const PtRgb *> pts((size_t)n);
    std::vector<int64_t> ns((size_t)n);
    for (int s = 0; s < n; s++) {
        if (!batch_pair_ok(c, "lmono_sor_filter_frames", "filters and map builders", s, sors, mbs)) return LMONO_EINVAL;
        if (!builder_last_cloud(c, "lmono_sor_filter_frames", mbs[s], pts[(size_t)s], ns[(size_t)s])) return LMONO_EINVAL;
    }
    return sor_filter_batch(c, "lmono_sor_filter_frames", n, sors, pts.data(), ns.data(), stats);
}

extern "C" int64_t lmono_sor_cloud(lmono_ctx *c, lmono_sor *s, lmono_point_rgb *out_h, int64_t cap)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    if (!out_h) return s->last_kept;
    return read_last(c, "lmono_sor_cloud", s->last_kept, cap, out_h, s->out, sizeof(PtRgb));
}

extern "C" int64_t lmono_sor_scores(lmono_ctx *c, lmono_sor *s, uint8_t *keep_h, uint32_t *v_h, int64_t cap)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    if (!keep_h && !v_h) return s->last_n;
    return read_last(c, "lmono_sor_scores", s->last_n, cap, keep_h, s->keep, 1, v_h, s->v, sizeof(uint32_t));
}

extern "C" int lmono_sor_threshold(lmono_ctx *c, lmono_sor *s, double out[3])
{
    if (!c || !s || s->ctx != c || !out) return LMONO_EINVAL;
    out[2] = sor_threshold((uint64_t)s->stats[3], (uint64_t)s->stats[5], (uint64_t)s->stats[6], (uint64_t)s->stats[7], s->mul, out[0], out[1]);
    return LMONO_OK;
}

extern "C" int lmono_sor_diag(lmono_ctx *c, lmono_sor *s, int64_t out[2])
{
    if (!c || !s || s->ctx != c || !out) return LMONO_EINVAL;
    out[0] = s->diag[0]; out[1] = s->diag[1];
    return LMONO_OK;
}

extern "C" int lmono_voxel_map_insert_filtered(lmono_ctx *c, int n, lmono_voxel_map *const *maps, lmono_sor *const *sors, int64_t *stats)
{
    if (!c || n <= 0 || !maps || !sors) return LMONO_EINVAL;
    std::vector<const PtRgb *> pts((size_t)n);
    std::vector<int64_t> ns((size_t)n);
    for (int s = 0; s < n; s++) {
        if (!batch_pair_ok(c, "lmono_voxel_map_insert_filtered", "maps and filters", s, maps, sors)) return LMONO_EINVAL;
        pts[(size_t)s] = sors[s]->out;
        ns[(size_t)s] = sors[s]->last_kept;
    }
    return vm_insert_batch(c, "lmono_voxel_map_insert_filtered", n, maps, pts.data(), ns.data(), stats);
}
