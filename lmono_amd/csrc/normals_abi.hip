// normals_abi.hip -- C ABI of the surface normals (included by lmono_hip.hip after icp_abi.hip: compute_frames reads a map builder, compute_map a voxel map)
#pragma once
#include "normals.hip"

struct lmono_normals {
    lmono_ctx *ctx = nullptr;
    int64_t max_points = 0;
    float r = 0.0f, r2 = 0.0f;
    int min_nb = 0;
    DevOwner mem;
    // the grid over the cloud (with an origin) and the cloud itself: every entry point brings its points into pts first; n_vox: the points
    // compute_map wrote there
    CellGrid grid;
    PtRgb *pts = nullptr;
    unsigned *n_vox = nullptr;
    // the last result
    NrmRecord *rec = nullptr;
    unsigned *count = nullptr;
    NrmDev *dev = nullptr;
    int64_t last_n = 0, stats[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    // per-call job table of a batch led by this handle
    NrmJob *jobs = nullptr;
    int jobs_cap = 0;
};

extern "C" void lmono_normals_destroy(lmono_normals *s) { delete s; }

extern "C" float lmono_normals_default_cell(float radius) { return nrm_default_cell(radius); }

extern "C" lmono_normals *lmono_normals_create(lmono_ctx *c, int64_t max_points, float radius, int min_neighbours, float cell, int max_rings)
{
    if (!c) return nullptr;
    if (max_points < 1 || max_points > kNrmMaxPoints || !nrm_params_ok(radius, min_neighbours, cell, max_rings)) {
        c->err = "lmono_normals_create: max_points in 1 .. 2^26, 0 < radius <= 4, min_neighbours >= 3, cell > 0 (with a finite 1 / cell), max_rings in 1 .. 64, "
                 "(max_rings - 0.25) cell >= radius";
        return nullptr;
    }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return nullptr; }
    lmono_normals *s = new lmono_normals();
    s->ctx = c;
    s->max_points = max_points;
    s->r = radius; s->r2 = radius * radius; s->min_nb = min_neighbours;
    const size_t n = (size_t)max_points;
    const bool ok = s->grid.alloc(s->mem, max_points, cell, max_rings, /*work_list=*/false) && s->mem.alloc_zero(s->n_vox, 1) && s->mem.alloc(s->pts, n) && s->mem.alloc(s->rec, n) &&
                    s->mem.alloc(s->count, n) && s->mem.alloc_zero(s->dev, 1);
    if (!ok) { c->err = "lmono_normals_create: device allocation failed"; lmono_normals_destroy(s); return nullptr; }
    return s;
}

static bool nrm_viewpoints_ok(const float *vps, int n)
{
    if (vps) for (int k = 0; k < 3 * n; k++) if (!std::isfinite(vps[k])) return false;
    return true;
}

// one compute for n handles whose clouds of ns[s] points (ns[s] <= max_points) are in flight into their pts buffers; vps: [n][3] or nullptr.
// One launch per phase for all streams: the five of the grid (cellgrid_build), k_nrm_compute, k_nrm_stats.  Ends synchronised.
static int nrm_compute_batch(lmono_ctx *c, const char *who, int n, lmono_normals *const *hs, const int64_t *ns, const float *vps, int64_t *stats)
{
    int64_t max_n = 0;
    // the handles show a result only once the call has ended well
    for (int s = 0; s < n; s++) {
        hs[s]->last_n = 0;
        for (int w = 0; w < 8; w++) hs[s]->stats[w] = 0;
        max_n = std::max(max_n, ns[s]);
    }
    auto finish = [&] {
        for (int s = 0; s < n; s++) {
            hs[s]->last_n = ns[s];
            hs[s]->stats[0] = ns[s];
            if (stats) std::memcpy(stats + 8 * s, hs[s]->stats, sizeof hs[s]->stats);
        }
        return LMONO_OK;
    };
    if (max_n == 0) return finish();                            // nothing to do: no launch
    lmono_normals *lead = hs[0];
    if (!lead->mem.grow_replace(lead->jobs, lead->jobs_cap, (size_t)n, /*floor=*/1)) { c->err = std::string(who) + ": job table allocation failed"; return LMONO_ENOMEM; }
    std::vector<NrmJob> jobs((size_t)n);
    for (int s = 0; s < n; s++) {
        const lmono_normals *f = hs[s];
        NrmJob &q = jobs[(size_t)s];
        q.g = f->grid.view(f->pts, ns[s]);
        q.rec = f->rec; q.count = f->count; q.dev = f->dev; q.r2 = f->r2; q.min_nb = f->min_nb; q.has_vp = vps ? 1 : 0;
        for (int a = 0; a < 3; a++) q.vp[a] = vps ? vps[3 * s + a] : 0.0f;
    }
    HIP_TRY(c, hipMemcpyAsync(lead->jobs, jobs.data(), sizeof(NrmJob) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (int rc = cellgrid_build</*kOrigin=*/true>(c, lead->jobs, n, max_n)) return rc;
    const dim3 g_pts((unsigned)((max_n + kNrmT - 1) / kNrmT), (unsigned)n);
    k_nrm_compute<<<g_pts, kNrmT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_nrm_compute")) return rc;
    k_nrm_stats<<<g_pts, kNrmT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_nrm_stats")) return rc;
    std::vector<CellWords> tg((size_t)n);
    std::vector<NrmDev> dev((size_t)n);
    for (int s = 0; s < n; s++) {
        if (ns[s] == 0) continue;
        HIP_TRY(c, hipMemcpyAsync(&tg[(size_t)s], hs[s]->grid.words, sizeof(CellWords), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&dev[(size_t)s], hs[s]->dev, sizeof(NrmDev), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int s = 0; s < n; s++) {
        if (ns[s] == 0) continue;
        const CellWords &t = tg[(size_t)s];
        const NrmDev &d = dev[(size_t)s];
        if ((int64_t)t.alloc + (int64_t)t.rejected != ns[s] || (int64_t)d.w[0] != (int64_t)t.rejected || (int64_t)(d.w[0] + d.w[1] + d.w[2]) != ns[s]) {
            c->err = std::string(who) + ": the placed, rejected and counted points do not add up to the cloud's size";
            return LMONO_ENODEV;
        }
        int64_t *st = hs[s]->stats;
        st[1] = (int64_t)d.w[0]; st[2] = (int64_t)d.w[1]; st[3] = (int64_t)d.w[2]; st[4] = (int64_t)d.w[3]; st[5] = (int64_t)d.w[4];
    }
    return finish();
}

extern "C" int lmono_normals_compute_d(lmono_ctx *c, lmono_normals *s, const lmono_point_rgb *pts_d, int64_t n, const float *viewpoint, int64_t *stats)
{
    if (!c || !s || s->ctx != c || n < 0 || (n > 0 && !pts_d)) return LMONO_EINVAL;
    if (!nrm_viewpoints_ok(viewpoint, 1)) { c->err = "lmono_normals_compute_d: non-finite viewpoint"; return LMONO_EINVAL; }
    if (n > s->max_points) { c->err = "lmono_normals_compute_d: more points than the handle's max_points"; return LMONO_ECAPACITY; }
    if (n > 0) HIP_TRY(c, hipMemcpyAsync(s->pts, pts_d, sizeof(PtRgb) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    return nrm_compute_batch(c, "lmono_normals_compute_d", 1, &s, &n, viewpoint, stats);
}

extern "C" int lmono_normals_compute(lmono_ctx *c, lmono_normals *s, const lmono_point_rgb *pts_h, int64_t n, const float *viewpoint, int64_t *stats)
{
    if (!c || !s || s->ctx != c || n < 0 || (n > 0 && !pts_h)) return LMONO_EINVAL;
    if (!nrm_viewpoints_ok(viewpoint, 1)) { c->err = "lmono_normals_compute: non-finite viewpoint"; return LMONO_EINVAL; }
    if (n > s->max_points) { c->err = "lmono_normals_compute: more points than the handle's max_points"; return LMONO_ECAPACITY; }
    if (n > 0) HIP_TRY(c, hipMemcpyAsync(s->pts, pts_h, sizeof(PtRgb) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    const int rc = nrm_compute_batch(c, "lmono_normals_compute", 1, &s, &n, viewpoint, stats);
    if (rc != LMONO_OK) (void)hipStreamSynchronize(c->stream);      // an early return must not leave the copy from the caller's buffer in flight
    return rc;
}

extern "C" int lmono_normals_compute_frames(lmono_ctx *c, int n, lmono_normals *const *hs, lmono_map_builder *const *mbs, const float *viewpoints, int64_t *stats)
{
    if (!c || n <= 0 || !hs || !mbs) return LMONO_EINVAL;
    if (n > 65535) { c->err = "lmono_normals_compute_frames: more than 65535 streams in one call"; return LMONO_EINVAL; }
    if (!nrm_viewpoints_ok(viewpoints, n)) { c->err = "lmono_normals_compute_frames: non-finite viewpoint"; return LMONO_EINVAL; }
    std::vector<const PtRgb *> pts((size_t)n);
    std::vector<int64_t> ns((size_t)n);
    for (int s = 0; s < n; s++) {
        if (!batch_pair_ok(c, "lmono_normals_compute_frames", "handles and map builders", s, hs, mbs)) return LMONO_EINVAL;
        if (!builder_last_cloud(c, "lmono_normals_compute_frames", mbs[s], pts[(size_t)s], ns[(size_t)s])) return LMONO_EINVAL;
        if (ns[(size_t)s] > hs[s]->max_points) { c->err = "lmono_normals_compute_frames: more points than the handle's max_points"; return LMONO_ECAPACITY; }
    }
    for (int s = 0; s < n; s++)
        if (ns[(size_t)s] > 0) HIP_TRY(c, hipMemcpyAsync(hs[s]->pts, pts[(size_t)s], sizeof(PtRgb) * (size_t)ns[(size_t)s], hipMemcpyDeviceToDevice, c->stream));
    return nrm_compute_batch(c, "lmono_normals_compute_frames", n, hs, ns.data(), viewpoints, stats);
}

extern "C" int lmono_normals_compute_map(lmono_ctx *c, lmono_normals *s, lmono_voxel_map *m, const float *viewpoint, int64_t *stats)
{
    if (!c || !s || s->ctx != c || !m || m->ctx != c) return LMONO_EINVAL;
    if (!nrm_viewpoints_ok(viewpoint, 1)) { c->err = "lmono_normals_compute_map: non-finite viewpoint"; return LMONO_EINVAL; }
    if (m->n_vox > s->max_points) { c->err = "lmono_normals_compute_map: more voxels than the handle's max_points"; return LMONO_ECAPACITY; }
    const int64_t n = m->n_vox;
    if (int rc = n > 0 ? vm_enqueue_points(c, m, s->pts, s->n_vox) : LMONO_OK) return rc;
    if (int rc = nrm_compute_batch(c, "lmono_normals_compute_map", 1, &s, &n, viewpoint, stats)) return rc;
    if (n > 0) {
        unsigned found = 0;
        HIP_TRY(c, hipMemcpy(&found, s->n_vox, sizeof found, hipMemcpyDeviceToHost));
        if ((int64_t)found != n) { s->last_n = 0; c->err = "lmono_normals_compute_map: the table's occupied records do not match the map's size"; return LMONO_ENODEV; }
    }
    return LMONO_OK;
}

extern "C" int64_t lmono_normals_read(lmono_ctx *c, lmono_normals *s, lmono_normal *out_h, uint32_t *count_h, int64_t cap)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    if (!out_h && !count_h) return s->last_n;
    return read_last(c, "lmono_normals_read", s->last_n, cap, out_h, s->rec, sizeof(NrmRecord), count_h, s->count, sizeof(unsigned));
}

extern "C" int64_t lmono_normals_cloud(lmono_ctx *c, lmono_normals *s, lmono_point_rgb *out_h, int64_t cap)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    if (!out_h) return s->last_n;
    return read_last(c, "lmono_normals_cloud", s->last_n, cap, out_h, s->pts, sizeof(PtRgb));
}
