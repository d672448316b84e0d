// sacia_abi.hip -- C ABI of the sample-consensus initial alignment (included by lmono_hip.hip after fpfh_abi.hip: an align reads the keypoints,
// descriptors and flags of two FPFH handles in device memory)
#pragma once
#include "sacia.hip"

struct lmono_sacia {
    lmono_ctx *ctx = nullptr;
    float msd = 0.0f, max_corr = 0.0f;
    int k_corr = 0, n_hyp = 0, launch_hyps = 0;
    uint32_t seed = 0;
    DevOwner mem;
    int *sl = nullptr, *tl = nullptr, *cand = nullptr;
    float *u = nullptr, *w = nullptr, *tpos = nullptr;
    unsigned long long *err = nullptr;
    unsigned *inl = nullptr;
    double *fit = nullptr;
    SaciaResult *res = nullptr;
    // the last result
    bool has = false;                       // a transform
    int64_t last_hyp = 0;                   // error words of the last align that ended well
    double T[12] = { 0 };
};

extern "C" void lmono_sacia_destroy(lmono_sacia *s) { delete s; }

extern "C" lmono_sacia *lmono_sacia_create(lmono_ctx *c, float min_sample_dist, float max_corr, int k_corr, int n_hyp, uint32_t seed, int launch_hyps)
{
    if (!c) return nullptr;
    if (!sacia_params_ok(min_sample_dist, max_corr, k_corr, n_hyp) || launch_hyps < 0) {
        c->err = "lmono_sacia_create: 0 <= min_sample_dist <= 4096, 0 < max_corr <= 16, k_corr in 1 .. 32, n_hyp in 1 .. 65536, launch_hyps >= 0";
        return nullptr;
    }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return nullptr; }
    lmono_sacia *s = new lmono_sacia();
    s->ctx = c;
    s->msd = min_sample_dist; s->max_corr = max_corr; s->k_corr = k_corr; s->n_hyp = n_hyp; s->seed = seed;
    s->launch_hyps = launch_hyps == 0 || launch_hyps > n_hyp ? n_hyp : launch_hyps;
    const size_t m = (size_t)kFpfhMaxKeypoints, nh = (size_t)n_hyp;
    const bool ok = s->mem.alloc(s->sl, m) && s->mem.alloc(s->tl, m) && s->mem.alloc(s->cand, m * (size_t)k_corr) && s->mem.alloc(s->u, 3 * m) && s->mem.alloc(s->w, 3 * m) &&
                    s->mem.alloc(s->tpos, 3 * m) && s->mem.alloc(s->err, nh) && s->mem.alloc(s->inl, nh) && s->mem.alloc(s->fit, 12 * nh) && s->mem.alloc_zero(s->res, 1);
    if (!ok) { c->err = "lmono_sacia_create: device allocation failed"; lmono_sacia_destroy(s); return nullptr; }
    return s;
}

// the usable keypoints of a handle: their indices and positions
static int sacia_side(lmono_ctx *c, const lmono_fpfh *f, std::vector<int> &list, std::vector<float> &pos)
{
    const size_t m = (size_t)f->last_m;
    std::vector<float> kp(3 * m);
    std::vector<unsigned> flag(m);
    HIP_TRY(c, hipMemcpyAsync(kp.data(), f->kp, sizeof(float) * 3 * m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(flag.data(), f->flag, sizeof(unsigned) * m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < m; k++)
        if (flag[k] == 1u) { list.push_back((int)k); pos.insert(pos.end(), kp.begin() + 3 * k, kp.begin() + 3 * k + 3); }
    return LMONO_OK;
}

static int sacia_align(lmono_ctx *c, lmono_sacia *s, lmono_fpfh *src, lmono_fpfh *tgt, int64_t *stats)
{
    const char *who = "lmono_sacia_align";
    if (src->last_m <= 0 || tgt->last_m <= 0) { c->err = std::string(who) + ": a descriptor handle without a result"; return LMONO_EINVAL; }
    std::vector<int> sl, tl;
    std::vector<float> sp, tp;
    if (int rc = sacia_side(c, src, sl, sp)) return rc;
    if (int rc = sacia_side(c, tgt, tl, tp)) return rc;
    const int ns = (int)sl.size(), nt = (int)tl.size();
    if (ns < 3 || nt < 3) { c->err = std::string(who) + ": fewer than 3 keypoints with a descriptor on a side"; return LMONO_EINVAL; }
    std::vector<float> u(sp.size()), w(tp.size());
    bool span = true;
    for (size_t e = 0; e < sp.size(); e++) { u[e] = sp[e] - sp[e % 3]; span = span && icp_in_span(u[e]); }
    for (size_t e = 0; e < tp.size(); e++) { w[e] = tp[e] - tp[e % 3]; span = span && icp_in_span(w[e]); }
    if (!span) { c->err = std::string(who) + ": a keypoint 2048 m or more from the first one of its side"; return LMONO_EINVAL; }
    SaciaJob q;
    q.sdesc = src->desc; q.tdesc = tgt->desc; q.sl = s->sl; q.tl = s->tl; q.u = s->u; q.w = s->w; q.tpos = s->tpos;
    q.ns = ns; q.nt = nt; q.K = s->k_corr < nt ? s->k_corr : nt; q.n_hyp = s->n_hyp; q.seed = s->seed;
    q.msd2 = s->msd * s->msd; q.mc2 = s->max_corr * s->max_corr;
    for (int a = 0; a < 3; a++) q.ct[a] = tp[a];
    q.cand = s->cand; q.err = s->err; q.inl = s->inl; q.fit = s->fit; q.res = s->res;
    HIP_TRY(c, hipMemcpyAsync(s->sl, sl.data(), sizeof(int) * (size_t)ns, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(s->tl, tl.data(), sizeof(int) * (size_t)nt, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(s->u, u.data(), sizeof(float) * u.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(s->w, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(s->tpos, tp.data(), sizeof(float) * tp.size(), hipMemcpyHostToDevice, c->stream));
    k_sacia_cand<<<(unsigned)ns, 64, 0, c->stream>>>(q);
    if (int rc = check_launch(c, "k_sacia_cand")) return rc;
    for (int h0 = 0; h0 < s->n_hyp; h0 += s->launch_hyps) {
        const int cnt = s->n_hyp - h0 < s->launch_hyps ? s->n_hyp - h0 : s->launch_hyps;
        k_sacia_hyp<<<(unsigned)cnt, kSaciaT, 0, c->stream>>>(q, h0);
        if (int rc = check_launch(c, "k_sacia_hyp")) return rc;
    }
    k_sacia_best<<<1, kSaciaT, 0, c->stream>>>(q);
    if (int rc = check_launch(c, "k_sacia_best")) return rc;
    SaciaResult r;
    HIP_TRY(c, hipMemcpyAsync(&r, s->res, sizeof r, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));                 // the uploads' host buffers live until here
    if (r.ok && (r.h < 0 || r.h >= s->n_hyp)) { c->err = std::string(who) + ": the winning hypothesis is out of range"; return LMONO_ENODEV; }
    if (r.ok) {
        double fit[12];
        HIP_TRY(c, hipMemcpyAsync(fit, s->fit + (size_t)r.h * 12, sizeof fit, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        sacia_transform(fit, fit + 9, sp.data(), tp.data(), s->T);
        s->has = true;
    }
    s->last_hyp = s->n_hyp;
    if (stats) {
        stats[0] = r.ok; stats[1] = r.h; stats[2] = (int64_t)r.err; stats[3] = r.inl; stats[4] = r.voids; stats[5] = ns; stats[6] = nt; stats[7] = s->n_hyp;
    }
    return LMONO_OK;
}

extern "C" int lmono_sacia_align(lmono_ctx *c, lmono_sacia *s, lmono_fpfh *src, lmono_fpfh *tgt, int64_t *stats)
{
    if (!c || !s || s->ctx != c || !src || !tgt || src->ctx != c || tgt->ctx != c) return LMONO_EINVAL;
    s->has = false; s->last_hyp = 0;                             // the handle shows a result only once the call has ended well
    const int rc = sacia_align(c, s, src, tgt, stats);
    if (rc != LMONO_OK) { (void)hipStreamSynchronize(c->stream); s->has = false; s->last_hyp = 0; }
    return rc;
}

extern "C" int lmono_sacia_transform(lmono_ctx *c, lmono_sacia *s, double out[12])
{
    if (!c || !s || s->ctx != c || !out) return LMONO_EINVAL;
    if (!s->has) { c->err = "lmono_sacia_transform: no transform (no align has ended with a hypothesis that is not void)"; return LMONO_EINVAL; }
    std::memcpy(out, s->T, sizeof s->T);
    return LMONO_OK;
}

extern "C" int64_t lmono_sacia_errors(lmono_ctx *c, lmono_sacia *s, uint64_t *err_h, uint32_t *inl_h, int64_t cap)
{
    if (!c || !s || s->ctx != c) return LMONO_EINVAL;
    if (!err_h && !inl_h) return s->last_hyp;
    return read_last(c, "lmono_sacia_errors", s->last_hyp, cap, err_h, s->err, sizeof(unsigned long long), inl_h, s->inl, sizeof(unsigned));
}
