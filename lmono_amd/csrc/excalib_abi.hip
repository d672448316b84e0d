// excalib_abi.hip -- C ABI of the camera-LiDAR rotation calibration (included by lmono_hip.hip behind posegraph_abi.hip): DESIGN.md 6i
#pragma once
#include "excalib.hip"

struct lmono_excalib {
    lmono_ctx *ctx = nullptr;
    int n_streams = 0;
    DevOwner mem;
    ExcState *state = nullptr;      // [n_streams]
};

namespace {

ExcState exc_fresh()
{
    ExcState s;
    memset(&s, 0, sizeof(s));
    exc_identity(s.rlc);
    return s;
}

bool exc_quats_ok(const double *q, int n)
{
    for (size_t e = 0; e < 4 * (size_t)n; e++) if (!std::isfinite(q[e])) return false;
    return true;
}

// Everything a call may be refused for, before anything is uploaded: -> LMONO_OK or the error with c->err set.  h == nullptr: the stateless call.
int exc_validate(lmono_ctx *c, const char *who, const lmono_excalib *h, int n, const int32_t *streams, const int32_t *m, const double *pairs,
                 const double *q_cam, const double *q_lidar, int count, size_t &total)
{
    total = 0;
    if (n < 1 || n > 65535) { c->err = std::string(who) + ": n outside 1..65535"; return LMONO_EINVAL; }
    if (m) {
        for (int s = 0; s < n; s++) {
            if (m[s] < 0) { c->err = std::string(who) + ": a pair count is negative"; return LMONO_EINVAL; }
            if (m[s] > kRejPts) { c->err = std::string(who) + ": a stream has more than 512 pairs"; return LMONO_ECAPACITY; }
            total += (size_t)m[s];
        }
        if (total > 0 && !pairs) { c->err = std::string(who) + ": pairs is null"; return LMONO_EINVAL; }
    }
    if (h) {
        if (count < 1) { c->err = std::string(who) + ": count below 1"; return LMONO_EINVAL; }
        if (!streams || !q_lidar || !exc_quats_ok(q_lidar, n) || (q_cam && !exc_quats_ok(q_cam, n))) {
            c->err = std::string(who) + ": a null array or a quaternion that is not finite"; return LMONO_EINVAL;
        }
        std::vector<char> seen((size_t)h->n_streams, 0);
        for (int s = 0; s < n; s++) {
            if (streams[s] < 0 || streams[s] >= h->n_streams) { c->err = std::string(who) + ": a stream index is out of range"; return LMONO_EINVAL; }
            // two workgroups would update one stream's state
            if (seen[(size_t)streams[s]]) { c->err = std::string(who) + ": a stream is named twice in one call"; return LMONO_EINVAL; }
            seen[(size_t)streams[s]] = 1;
        }
    }
    return LMONO_OK;
}

// one launch over n streams: mode bits per the arguments given (m: stages 1-3, h: stage 4)
int exc_run(lmono_ctx *c, const char *who, lmono_excalib *h, int n, const int32_t *streams, const int32_t *m, const double *pairs, const double *q_cam,
            const double *q_lidar, int count, double *R_cam_h, int32_t *stats_h, double *rlc_h, double *sv_h, double *huber_h, int32_t *ok_h)
{
    size_t total = 0;
    if (int rc = exc_validate(c, who, h, n, streams, m, pairs, q_cam, q_lidar, count, total)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf buf(c);
    bool ok = true;
    const double *pairs_d = m ? buf.up(pairs, total * 4, ok) : nullptr;
    // results of one stream, adjacent: R_cam 9, rlc 9, sv 4, huber 1 doubles; stats 6, ok 1 ints
    double *res_d = buf.up((const double *)nullptr, (size_t)n * 23, ok);
    int *res_i = buf.up((const int *)nullptr, (size_t)n * 7, ok);
    if (!ok) { c->err = std::string(who) + ": device allocation failed"; return LMONO_ENOMEM; }
    std::vector<ExcJob> jobs((size_t)n);
    size_t at = 0;
    for (int s = 0; s < n; s++) {
        ExcJob &j = jobs[(size_t)s];
        memset(&j, 0, sizeof(j));
        j.pairs = m ? pairs_d + 4 * at : nullptr; j.m = m ? m[s] : 0; j.mode = (m ? kExcRel : 0) | (h ? kExcCal : 0); j.count = count;
        for (int e = 0; e < 4; e++) { j.q_cam[e] = q_cam ? q_cam[4 * (size_t)s + e] : 0.0; j.q_lidar[e] = q_lidar ? q_lidar[4 * (size_t)s + e] : 0.0; }
        j.state = h ? h->state + streams[s] : nullptr;
        double *d = res_d + 23 * (size_t)s;
        int *i = res_i + 7 * (size_t)s;
        j.R_cam = d; j.rlc = d + 9; j.sv = d + 18; j.huber = d + 22; j.stats = i; j.ok = i + 6;
        at += m ? (size_t)m[s] : 0;
    }
    const ExcJob *jobs_d = buf.up(jobs.data(), jobs.size(), ok);
    buf.ready(ok);
    if (!ok) { c->err = std::string(who) + ": upload failed"; return LMONO_ENOMEM; }
    k_excalib_step<<<(unsigned)n, kExcT, 0, c->stream>>>(jobs_d);
    if (int rc = check_launch(c, "k_excalib_step")) return rc;
    std::vector<double> rd((size_t)n * 23);
    std::vector<int> ri((size_t)n * 7);
    if (!buf.down(rd.data(), res_d, sizeof(double) * rd.size()) || !buf.down(ri.data(), res_i, sizeof(int) * ri.size()) || !buf.fetch()) {
        c->err = std::string(who) + ": read-back failed"; return LMONO_ENODEV;
    }
    for (int s = 0; s < n; s++) {
        const double *d = &rd[23 * (size_t)s];
        const int *i = &ri[7 * (size_t)s];
        if (m && R_cam_h) for (int e = 0; e < 9; e++) R_cam_h[9 * (size_t)s + e] = d[e];
        if (m && stats_h) for (int e = 0; e < 6; e++) stats_h[6 * (size_t)s + e] = i[e];
        if (h && rlc_h) for (int e = 0; e < 9; e++) rlc_h[9 * (size_t)s + e] = d[9 + e];
        if (h && sv_h) for (int e = 0; e < 4; e++) sv_h[4 * (size_t)s + e] = d[18 + e];
        if (h && huber_h) huber_h[s] = d[22];
        if (h && ok_h) ok_h[s] = i[6];
    }
    return LMONO_OK;
}

} // namespace

extern "C" int lmono_excalib_create(lmono_ctx *c, int n_streams, lmono_excalib **out)
{
    if (!c || !out || n_streams < 1 || n_streams > 65535) return LMONO_EINVAL;
    *out = nullptr;
    HIP_TRY(c, hipSetDevice(c->device));
    std::unique_ptr<lmono_excalib> h(new lmono_excalib());
    h->ctx = c; h->n_streams = n_streams;
    if (!h->mem.alloc(h->state, (size_t)n_streams)) { c->err = "lmono_excalib_create: device allocation failed"; return LMONO_ENOMEM; }
    if (int rc = lmono_excalib_reset(h.get(), -1)) return rc;
    *out = h.release();
    return LMONO_OK;
}

extern "C" void lmono_excalib_destroy(lmono_excalib *h)
{
    if (!h) return;
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
}

extern "C" int lmono_excalib_reset(lmono_excalib *h, int stream)
{
    if (!h || stream < -1 || stream >= h->n_streams) return LMONO_EINVAL;
    lmono_ctx *c = h->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    const int first = stream < 0 ? 0 : stream, cnt = stream < 0 ? h->n_streams : 1;
    const std::vector<ExcState> fresh((size_t)cnt, exc_fresh());
    HIP_TRY(c, hipMemcpyAsync(h->state + first, fresh.data(), sizeof(ExcState) * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // `fresh` is read by the copy until here
    return LMONO_OK;
}

extern "C" int lmono_relative_rotation(lmono_ctx *c, int n, const int32_t *m, const double *pairs, double *R_out, int32_t *stats)
{
    if (!c || !m) return LMONO_EINVAL;
    return exc_run(c, "lmono_relative_rotation", nullptr, n, nullptr, m, pairs, nullptr, nullptr, 1, R_out, stats, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int lmono_excalib_push(lmono_excalib *h, int n, const int32_t *streams, const double *q_cam, const double *q_lidar, int count, double *rlc, double *sv,
                                  double *huber, int32_t *ok)
{
    if (!h) return LMONO_EINVAL;
    if (!q_cam) { h->ctx->err = "lmono_excalib_push: q_cam is null"; return LMONO_EINVAL; }
    return exc_run(h->ctx, "lmono_excalib_push", h, n, streams, nullptr, nullptr, q_cam, q_lidar, count, nullptr, nullptr, rlc, sv, huber, ok);
}

extern "C" int lmono_excalib_step(lmono_excalib *h, int n, const int32_t *streams, const int32_t *m, const double *pairs, const double *q_lidar, int count,
                                  double *R_cam, int32_t *stats, double *rlc, double *sv, double *huber, int32_t *ok)
{
    if (!h) return LMONO_EINVAL;
    if (!m) { h->ctx->err = "lmono_excalib_step: m is null"; return LMONO_EINVAL; }
    return exc_run(h->ctx, "lmono_excalib_step", h, n, streams, m, pairs, nullptr, q_lidar, count, R_cam, stats, rlc, sv, huber, ok);
}

extern "C" int lmono_excalib_state(lmono_excalib *h, int stream, int *frame_count, double *M, double *rlc)
{
    if (!h || stream < 0 || stream >= h->n_streams) return LMONO_EINVAL;
    lmono_ctx *c = h->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    ExcState s;
    HIP_TRY(c, hipMemcpyAsync(&s, h->state + stream, sizeof(s), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (frame_count) *frame_count = s.frame_count;
    if (M) for (int e = 0; e < 16; e++) M[e] = s.M[e];
    if (rlc) for (int e = 0; e < 9; e++) rlc[e] = s.rlc[e];
    return LMONO_OK;
}
