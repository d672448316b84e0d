// fpfh_abi.hip -- C ABI of the FPFH descriptors (included by lmono_hip.hip after normals_abi.hip: a compute reads a normals handle's cloud and records)
#pragma once
#include "fpfh.hip"

struct lmono_fpfh {
    lmono_ctx *ctx = nullptr;
    int64_t max_points = 0, max_keypoints = 0;
    float r = 0.0f, r2 = 0.0f;
    DevOwner mem;
    CellGrid grid;                          // over the normals handle's cloud, with an origin
    unsigned *need = nullptr, *list = nullptr, *spfh = nullptr;
    // the last result
    float *kp = nullptr, *desc = nullptr;
    unsigned *nb = nullptr, *flag = nullptr;
    FpfhDev *dev = nullptr;
    int64_t last_m = 0, stats[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    // per-call job table of a batch led by this handle
    FpfhJob *jobs = nullptr;
    int jobs_cap = 0;
};

extern "C" void lmono_fpfh_destroy(lmono_fpfh *s) { delete s; }

extern "C" float lmono_fpfh_default_cell(float radius) { return fpfh_default_cell(radius); }

extern "C" lmono_fpfh *lmono_fpfh_create(lmono_ctx *c, int64_t max_points, int64_t max_keypoints, float radius, float cell, int max_rings)
{
    if (!c) return nullptr;
    if (max_points < 1 || max_points > kFpfhMaxPoints || max_keypoints < 1 || max_keypoints > kFpfhMaxKeypoints || !fpfh_params_ok(radius, cell, max_rings)) {
        c->err = "lmono_fpfh_create: max_points in 1 .. 2^26, max_keypoints in 1 .. 4096, 0 < radius <= 4, cell > 0 (with a finite 1 / cell), max_rings in 1 .. 64, "
                 "(max_rings - 0.25) cell >= radius";
        return nullptr;
    }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return nullptr; }
    lmono_fpfh *s = new lmono_fpfh();
    s->ctx = c;
    s->max_points = max_points; s->max_keypoints = max_keypoints;
    s->r = radius; s->r2 = radius * radius;
    const size_t n = (size_t)max_points, m = (size_t)max_keypoints;
    const bool ok = s->grid.alloc(s->mem, max_points, cell, max_rings, /*work_list=*/false) && s->mem.alloc(s->need, n) && s->mem.alloc(s->list, n) &&
                    s->mem.alloc(s->spfh, n * kFpfhRow) && s->mem.alloc(s->kp, 3 * m) && s->mem.alloc(s->desc, m * kFpfhDim) && s->mem.alloc(s->nb, m) &&
                    s->mem.alloc(s->flag, m) && s->mem.alloc_zero(s->dev, 1);
    if (!ok) { c->err = "lmono_fpfh_create: device allocation failed"; lmono_fpfh_destroy(s); return nullptr; }
    return s;
}

// One compute for n handles, each over the cloud and records of a normals handle and ms[s] keypoints on the host.  One launch per phase for
// all streams: the five of the grid (cellgrid_build), k_fpfh_clear, k_fpfh_mark, k_fpfh_spfh, k_fpfh_weight.  Ends synchronised.
static int fpfh_compute_batch(lmono_ctx *c, const char *who, int n, lmono_fpfh *const *hs, lmono_normals *const *nhs, const float *const *kps, const int64_t *ms, int64_t *stats)
{
    int64_t max_n = 0, max_m = 0;
    for (int s = 0; s < n; s++) {
        const int fa = batch_handle_fault(c, s, hs);
        if (fa == kHandleForeign || !nhs[s] || nhs[s]->ctx != c || ms[s] < 0 || (ms[s] > 0 && !kps[s])) { c->err = std::string(who) + ": bad stream arguments"; return LMONO_EINVAL; }
        if (fa == kHandleRepeated) { c->err = std::string(who) + ": descriptor handles must be distinct"; return LMONO_EINVAL; }
        if (nhs[s]->last_n <= 0) { c->err = std::string(who) + ": a normals handle without a result"; return LMONO_EINVAL; }
        if (nhs[s]->last_n > hs[s]->max_points) { c->err = std::string(who) + ": more points than the handle's max_points"; return LMONO_ECAPACITY; }
        if (ms[s] > hs[s]->max_keypoints) { c->err = std::string(who) + ": more keypoints than the handle's max_keypoints"; return LMONO_ECAPACITY; }
        for (int64_t k = 0; k < 3 * ms[s]; k++)
            if (!std::isfinite(kps[s][k])) { c->err = std::string(who) + ": non-finite keypoint"; return LMONO_EINVAL; }
        max_n = std::max(max_n, nhs[s]->last_n); max_m = std::max(max_m, ms[s]);
    }
    // the handles show a result only once the call has ended well
    for (int s = 0; s < n; s++) {
        hs[s]->last_m = 0;
        for (int w = 0; w < 8; w++) hs[s]->stats[w] = 0;
    }
    auto finish = [&] {
        for (int s = 0; s < n; s++) {
            hs[s]->last_m = ms[s];
            hs[s]->stats[0] = ms[s];
            if (stats) std::memcpy(stats + 8 * s, hs[s]->stats, sizeof hs[s]->stats);
        }
        return LMONO_OK;
    };
    if (max_m == 0) return finish();                            // nothing to do: no launch
    lmono_fpfh *lead = hs[0];
    if (!lead->mem.grow_replace(lead->jobs, lead->jobs_cap, (size_t)n, /*floor=*/1)) { c->err = std::string(who) + ": job table allocation failed"; return LMONO_ENOMEM; }
    std::vector<FpfhJob> jobs((size_t)n);
    for (int s = 0; s < n; s++) {
        const lmono_fpfh *f = hs[s];
        FpfhJob &q = jobs[(size_t)s];
        q.g = f->grid.view(nhs[s]->pts, nhs[s]->last_n);
        q.rec = nhs[s]->rec; q.kp = f->kp; q.m = (int)ms[s]; q.r2 = f->r2;
        q.need = f->need; q.list = f->list; q.spfh = f->spfh; q.desc = f->desc; q.nb = f->nb; q.flag = f->flag; q.dev = f->dev;
        if (ms[s] > 0) HIP_TRY(c, hipMemcpyAsync(f->kp, kps[s], sizeof(float) * 3 * (size_t)ms[s], hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(lead->jobs, jobs.data(), sizeof(FpfhJob) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (int rc = cellgrid_build</*kOrigin=*/true>(c, lead->jobs, n, max_n)) return rc;
    const dim3 g_pts((unsigned)((max_n + kCellT - 1) / kCellT), (unsigned)n), g_mark((unsigned)((max_m + kFpfhMarkT / 64 - 1) / (kFpfhMarkT / 64)), (unsigned)n);
    const dim3 g_spfh((unsigned)((max_n + kFpfhT - 1) / kFpfhT), (unsigned)n), g_kp((unsigned)max_m, (unsigned)n);
    k_fpfh_clear<<<g_pts, kCellT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_fpfh_clear")) return rc;
    k_fpfh_mark<<<g_mark, kFpfhMarkT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_fpfh_mark")) return rc;
    k_fpfh_spfh<<<g_spfh, kFpfhT, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_fpfh_spfh")) return rc;
    k_fpfh_weight<<<g_kp, 64, 0, c->stream>>>(lead->jobs);
    if (int rc = check_launch(c, "k_fpfh_weight")) return rc;
    std::vector<FpfhDev> dev((size_t)n);
    for (int s = 0; s < n; s++)
        HIP_TRY(c, hipMemcpyAsync(&dev[(size_t)s], hs[s]->dev, sizeof(FpfhDev), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int s = 0; s < n; s++) {
        const FpfhDev &d = dev[(size_t)s];
        if ((int64_t)d.w[0] > nhs[s]->last_n) { c->err = std::string(who) + ": the list of needed points is longer than the cloud"; return LMONO_ENODEV; }
        if ((int64_t)(d.w[3] + d.w[4]) != ms[s]) {
            c->err = std::string(who) + ": the keypoints with and without a descriptor do not add up to the keypoints";
            return LMONO_ENODEV;
        }
        int64_t *st = hs[s]->stats;
        st[1] = (int64_t)d.w[3]; st[2] = (int64_t)d.w[4]; st[3] = (int64_t)d.w[0]; st[4] = (int64_t)d.w[1]; st[5] = (int64_t)d.w[2]; st[6] = (int64_t)d.w[5]; st[7] = (int64_t)d.w[6];
    }
    return finish();
}

extern "C" int lmono_fpfh_compute_batch(lmono_ctx *c, int n, lmono_fpfh *const *fpfhs, lmono_normals *const *normals, const float *const *keypoints_h, const int64_t *ms, int64_t *stats)
{
    if (!c || n <= 0 || !fpfhs || !normals || !keypoints_h || !ms) return LMONO_EINVAL;
    if (n > 65535) { c->err = "lmono_fpfh_compute_batch: more than 65535 streams in one call"; return LMONO_EINVAL; }
    const int rc = fpfh_compute_batch(c, "lmono_fpfh_compute_batch", n, fpfhs, normals, keypoints_h, ms, stats);
    if (rc != LMONO_OK) (void)hipStreamSynchronize(c->stream);      // an early return must not leave a copy from the caller's buffers in flight
    return rc;
}

extern "C" int lmono_fpfh_compute(lmono_ctx *c, lmono_fpfh *s, lmono_normals *normals, const float *keypoints_h, int64_t m, int64_t *stats)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    const int rc = fpfh_compute_batch(c, "lmono_fpfh_compute", 1, &s, &normals, &keypoints_h, &m, stats);
    if (rc != LMONO_OK) (void)hipStreamSynchronize(c->stream);
    return rc;
}

extern "C" int64_t lmono_fpfh_read(lmono_ctx *c, lmono_fpfh *s, float *desc_h, uint32_t *count_h, uint32_t *flag_h, int64_t cap)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    if (!desc_h && !count_h && !flag_h) return s->last_m;
    const int64_t rc = read_last(c, "lmono_fpfh_read", s->last_m, cap, desc_h, s->desc, sizeof(float) * kFpfhDim, count_h, s->nb, sizeof(unsigned));
    if (rc < 0 || !flag_h) return rc;
    return read_last(c, "lmono_fpfh_read", s->last_m, cap, flag_h, s->flag, sizeof(unsigned));
}

extern "C" int64_t lmono_fpfh_keypoints(lmono_ctx *c, lmono_fpfh *s, float *out_h, int64_t cap)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    if (!out_h) return s->last_m;
    return read_last(c, "lmono_fpfh_keypoints", s->last_m, cap, out_h, s->kp, sizeof(float) * 3);
}
