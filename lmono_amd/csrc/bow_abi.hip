// bow_abi.hip -- C ABI of the loop detector's database (included by lmono_hip.hip behind keyframe_abi.hip): DESIGN.md 6h
#pragma once
#include "bow.hip"

struct lmono_brief_vocabulary {
    lmono_ctx *ctx = nullptr;
    std::shared_ptr<BowVocDev> dev;
    // scratch of lmono_brief_vocabulary_transform, grown to the largest n seen
    DevOwner mem;
    uint32_t *t_desc = nullptr;
    int *t_word = nullptr;
    double *t_weight = nullptr;
    BowWordsJob *t_job = nullptr;
    int t_cap = 0;
};

// replaces BriefVocabulary::loadBin (ThirdParty/DVision + VocabularyBinary.hpp, TemplatedVocabulary.h:1500-1560) as LoopDetector::loadVocabulary calls it (LoopDetector.cc:26-31)
extern "C" lmono_brief_vocabulary *lmono_brief_vocabulary_create(lmono_ctx *c, int k, int L, int scoring, int weighting, int n_nodes, const int32_t *node_id, const int32_t *parent_id,
                                                                 const double *weight, const uint32_t *descriptors, int n_words, const int32_t *word_node_id, const int32_t *word_id)
{
    if (!c) return nullptr;
    BowVocHost h;
    if (const char *why = bow_voc_build(k, L, scoring, weighting, n_nodes, node_id, parent_id, weight, descriptors, n_words, word_node_id, word_id, h)) { c->err = why; return nullptr; }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return nullptr; }
    auto dev = std::make_shared<BowVocDev>();
    dev->ctx = c;
    BowVoc &v = dev->v;
    v.n_nodes = h.n_nodes; v.n_words = h.n_words; v.k = h.k; v.L = h.L;
    if (!(dev->mem.upload(v.desc, h.desc) && dev->mem.upload(v.child_begin, h.child_begin) && dev->mem.upload(v.child_count, h.child_count) && dev->mem.upload(v.word, h.word) &&
          dev->mem.upload(v.weight, h.weight))) { c->err = "lmono_brief_vocabulary_create: device allocation failed"; return nullptr; }
    lmono_brief_vocabulary *voc = new lmono_brief_vocabulary();
    voc->ctx = c; voc->dev = dev;
    return voc;
}

// the handle goes; the device tree stays while a store still holds it
extern "C" void lmono_brief_vocabulary_destroy(lmono_brief_vocabulary *voc) { delete voc; }

// replaces TemplatedVocabulary::transform(feature, word_id, weight) (TemplatedVocabulary.h:1217-1258)
extern "C" int lmono_brief_vocabulary_transform(lmono_ctx *c, lmono_brief_vocabulary *voc, int n, const uint32_t *desc_h, int32_t *word_h, double *weight_h)
{
    if (!c || !voc || voc->ctx != c || n < 0 || (n > 0 && !desc_h)) return LMONO_EINVAL;
    if (n == 0) return LMONO_OK;
    if (n > 65535 * kBowT) { c->err = "lmono_brief_vocabulary_transform: more than 16776960 descriptors in one call"; return LMONO_ECAPACITY; }
    if (voc->t_cap < n) {
        const int old = voc->t_cap;
        int cap = 0;
        voc->t_cap = 0;
        auto grow = [&](auto *&p, size_t per) { cap = old; return voc->mem.grow_replace(p, cap, (size_t)n, /*floor=*/64, per); };
        if (!grow(voc->t_desc, 8) || !grow(voc->t_word, 1) || !grow(voc->t_weight, 1)) { c->err = "lmono_brief_vocabulary_transform: device allocation failed"; return LMONO_ENOMEM; }
        voc->t_cap = cap;
    }
    if (!voc->t_job && !voc->mem.alloc(voc->t_job, 1)) { c->err = "lmono_brief_vocabulary_transform: device allocation failed"; return LMONO_ENOMEM; }
    const BowWordsJob job{ voc->t_desc, n, voc->t_word, voc->t_weight };
    HIP_TRY(c, hipMemcpyAsync(voc->t_desc, desc_h, 32 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(voc->t_job, &job, sizeof(job), hipMemcpyHostToDevice, c->stream));
    k_bow_words<<<dim3(1u, (unsigned)((n + kBowT - 1) / kBowT)), kBowT, 0, c->stream>>>(voc->dev->v, voc->t_job);
    const int rc = check_launch(c, "k_bow_words");
    if (rc == LMONO_OK && word_h) HIP_TRY(c, hipMemcpyAsync(word_h, voc->t_word, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (rc == LMONO_OK && weight_h) HIP_TRY(c, hipMemcpyAsync(weight_h, voc->t_weight, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));                // `job` is read by the copy until here
    return rc;
}

// replaces LoopDetector::loadVocabulary's db.setVocabulary(*voc, false, 0) (LoopDetector.cc:29)
extern "C" int lmono_keyframes_set_vocabulary(lmono_ctx *c, lmono_keyframes *k, lmono_brief_vocabulary *voc)
{
    if (!c || !k || k->ctx != c || (voc && voc->ctx != c)) return LMONO_EINVAL;
    if (!voc) {
        k->voc.reset(); k->bow_done = 0;
        k->mem.release(k->bow_word); k->mem.release(k->bow_val); k->mem.release(k->bow_n); k->mem.release(k->q_s); k->mem.release(k->q_flag);
        return LMONO_OK;
    }
    if (k->max_kp > kBowMaxKp) { c->err = "lmono_keyframes_set_vocabulary: the BoW sort holds 16384 corners per keyframe, the store was created with a larger max_keypoints"; return LMONO_ECAPACITY; }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return LMONO_ENODEV; }
    if (!k->bow_word) {
        const size_t slots = (size_t)k->max_kf, per = (size_t)k->max_kp;
        DevOwner &m = k->mem;
        if (!(m.alloc(k->bow_word, slots * per) && m.alloc(k->bow_val, slots * per) && m.alloc_zero(k->bow_n, slots) && m.alloc(k->q_s, slots) && m.alloc(k->q_flag, slots))) {
            m.release(k->bow_word); m.release(k->bow_val); m.release(k->bow_n); m.release(k->q_s); m.release(k->q_flag);
            c->err = "lmono_keyframes_set_vocabulary: device allocation failed"; return LMONO_ENOMEM;
        }
    }
    // the sort of 16384 word ids takes the whole 64 KiB a kernel may ask for as dynamic LDS, beside the kernel's static arrays
    HIP_TRY(c, hipFuncSetAttribute((const void *)k_bow_vector, hipFuncAttributeMaxDynamicSharedMemorySize, kBowMaxKp * (int)sizeof(int)));
    k->voc = voc->dev; k->bow_done = 0;
    return LMONO_OK;
}

// The BoW vectors of every stored keyframe beyond the watermark of each store, queued on the stream: one k_bow_words and one
// k_bow_vector launch over all of them.  The stores are the caller's to check (distinct, one vocabulary)
static int bow_build(lmono_ctx *c, int n, lmono_keyframes *const *kfs)
{
    size_t pending = 0;
    for (int s = 0; s < n; s++) pending += (size_t)(kfs[s]->n_kf - kfs[s]->bow_done);
    if (pending == 0) return LMONO_OK;
    lmono_keyframes *lead = kfs[0];
    if (lead->b_cap < 0 || (size_t)lead->b_cap < pending) {
        const int old = lead->b_cap;
        int cap = 0;
        lead->b_cap = 0;
        auto grow = [&](auto *&p) { cap = old; return lead->mem.grow_replace(p, cap, pending, /*floor=*/16); };
        if (!grow(lead->b_wjobs) || !grow(lead->b_vjobs)) { c->err = "lmono_keyframes_bow: job table allocation failed"; return LMONO_ENOMEM; }
        lead->b_cap = cap;
    }
    std::vector<BowWordsJob> wj; std::vector<BowVecJob> vj;
    wj.reserve(pending); vj.reserve(pending);
    int max_n = 1;
    for (int s = 0; s < n; s++) {
        lmono_keyframes *k = kfs[s];
        const size_t per = (size_t)k->max_kp;
        for (int f = k->bow_done; f < k->n_kf; f++) {
            const size_t slot = (size_t)f;
            const int nk = std::min(std::max(k->n_kp_h[slot], 0), k->max_kp);
            wj.push_back(BowWordsJob{ k->desc + slot * per * 8, nk, k->bow_word + slot * per, nullptr });
            vj.push_back(BowVecJob{ nk, k->bow_word + slot * per, k->bow_val + slot * per, k->bow_n + slot });
            max_n = std::max(max_n, nk);
        }
    }
    const int lds_ints = bow_pow2(max_n);
    if (lds_ints > kBowMaxKp) { c->err = "lmono_keyframes_bow: a keyframe has more than 16384 corners"; return LMONO_ECAPACITY; }
    HIP_TRY(c, hipMemcpyAsync(lead->b_wjobs, wj.data(), sizeof(BowWordsJob) * pending, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(lead->b_vjobs, vj.data(), sizeof(BowVecJob) * pending, hipMemcpyHostToDevice, c->stream));
    const BowVoc &v = lead->voc->v;
    k_bow_words<<<dim3((unsigned)pending, (unsigned)((max_n + kBowT - 1) / kBowT)), kBowT, 0, c->stream>>>(v, lead->b_wjobs);
    int rc = check_launch(c, "k_bow_words");
    if (rc == LMONO_OK) {
        k_bow_vector<<<(unsigned)pending, kBowT, sizeof(int) * (size_t)lds_ints, c->stream>>>(v, lead->b_vjobs, lds_ints);
        rc = check_launch(c, "k_bow_vector");
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));                // the job tables' sources (wj, vj) go with this scope
    if (rc != LMONO_OK) return rc;
    for (int s = 0; s < n; s++) kfs[s]->bow_done = kfs[s]->n_kf;
    return LMONO_OK;
}

static int bow_store_fault(lmono_ctx *c, const lmono_keyframes *k, int cur, const char *who)
{
    if (!k->voc) { c->err = std::string(who) + ": no vocabulary is attached to the store (lmono_keyframes_set_vocabulary)"; return LMONO_EINVAL; }
    if (cur < 0 || cur >= k->n_kf) { c->err = std::string(who) + ": the keyframe index is not a stored keyframe"; return LMONO_EINVAL; }
    return LMONO_OK;
}

// db.query of keyframe cur[s] of every store: vectors brought up to date, then k_bow_score and k_bow_top once over all streams, one
// read-back into out [n].  Everything is checked by the caller
static int bow_query(lmono_ctx *c, int n, lmono_keyframes *const *kfs, const int *cur, const int *max_id, int max_results, BowResult *out)
{
    if (int rc = bow_build(c, n, kfs)) return rc;
    lmono_keyframes *lead = kfs[0];
    if (lead->q_cap < n) {
        const int old = lead->q_cap;
        int cap = 0;
        lead->q_cap = 0;
        auto grow = [&](auto *&p) { cap = old; return lead->mem.grow_replace(p, cap, (size_t)n, /*floor=*/1); };
        if (!grow(lead->q_jobs) || !grow(lead->q_out)) { c->err = "lmono_keyframes_query: job table allocation failed"; return LMONO_ENOMEM; }
        lead->q_cap = cap;
    }
    std::vector<BowQueryJob> jobs((size_t)n);
    int max_cur = 1;
    for (int s = 0; s < n; s++) {
        lmono_keyframes *k = kfs[s];
        jobs[(size_t)s] = BowQueryJob{ k->bow_word, k->bow_val, k->bow_n, k->max_kp, k->n_kf, cur[s], max_id[s], max_results, k->q_s, k->q_flag, lead->q_out + s };
        max_cur = std::max(max_cur, cur[s]);
    }
    HIP_TRY(c, hipMemcpyAsync(lead->q_jobs, jobs.data(), sizeof(BowQueryJob) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    k_bow_score<<<dim3((unsigned)((max_cur + kBowScoreT - 1) / kBowScoreT), (unsigned)n), kBowScoreT, 0, c->stream>>>(lead->q_jobs);
    int rc = check_launch(c, "k_bow_score");
    if (rc == LMONO_OK) {
        k_bow_top<<<(unsigned)n, kBowT, 0, c->stream>>>(lead->q_jobs);
        rc = check_launch(c, "k_bow_top");
    }
    if (rc == LMONO_OK) HIP_TRY(c, hipMemcpyAsync(out, lead->q_out, sizeof(BowResult) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (rc != LMONO_OK) return rc;
    for (int s = 0; s < n; s++) out[s].n = std::min(std::max(out[s].n, 0), max_results);
    return LMONO_OK;
}

// replaces TemplatedVocabulary::transform(features, BowVector &) with TF_IDF / L1_NORM (TemplatedVocabulary.h:1065-1121), as db.add and db.query call it
extern "C" int lmono_keyframes_bow(lmono_ctx *c, lmono_keyframes *k, int index, int *n_out, int32_t *word_h, double *value_h)
{
    if (!c || !k || k->ctx != c) return LMONO_EINVAL;
    if (int rc = bow_store_fault(c, k, index, "lmono_keyframes_bow")) return rc;
    if (int rc = bow_build(c, 1, &k)) return rc;
    int m = 0;
    HIP_TRY(c, hipMemcpyAsync(&m, k->bow_n + index, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    m = std::min(std::max(m, 0), k->n_kp_h[(size_t)index]);
    const size_t at = (size_t)index * (size_t)k->max_kp;
    if (m && word_h) HIP_TRY(c, hipMemcpyAsync(word_h, k->bow_word + at, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (m && value_h) HIP_TRY(c, hipMemcpyAsync(value_h, k->bow_val + at, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n_out) *n_out = m;
    return LMONO_OK;
}

// replaces db.query(brief_descriptors, ret, max_results, max_id) (TemplatedDatabase.h:610-723, queryL1) for the keyframes stored before cur
extern "C" int lmono_keyframes_query(lmono_ctx *c, lmono_keyframes *k, int cur, int max_results, int max_id, int *n_out, int32_t *id_h, double *score_h)
{
    if (!c || !k || k->ctx != c) return LMONO_EINVAL;
    if (int rc = bow_store_fault(c, k, cur, "lmono_keyframes_query")) return rc;
    if (max_results < 1 || max_results > kBowMaxResults) { c->err = "lmono_keyframes_query: max_results outside 1..16"; return LMONO_EINVAL; }
    BowResult r;
    if (int rc = bow_query(c, 1, &k, &cur, &max_id, max_results, &r)) return rc;
    if (n_out) *n_out = r.n;
    for (int i = 0; i < r.n; i++) { if (id_h) id_h[i] = r.id[i]; if (score_h) score_h[i] = r.score[i]; }
    return LMONO_OK;
}

// replaces LoopDetector::detectLoop (LoopDetector.cc:167-260) for n stores at once; the stored keyframes are the database, so db.add is the store's add
extern "C" int lmono_keyframes_detect_loop_batch(lmono_ctx *c, int n, lmono_keyframes *const *kfs, const int *cur, int loop_search_gap, int *loop_index_out, int *n_out,
                                                 int32_t *id_h, double *score_h)
{
    if (!c || n <= 0 || n > 65535 || !kfs || !cur) return LMONO_EINVAL;
    for (int s = 0; s < n; s++) {
        const int fault = batch_handle_fault(c, s, kfs);
        if (fault == kHandleForeign) { c->err = "lmono_keyframes_detect_loop_batch: a null store or one of another context"; return LMONO_EINVAL; }
        if (fault == kHandleRepeated) { c->err = "lmono_keyframes_detect_loop_batch: stores must be distinct"; return LMONO_EINVAL; }
        if (int rc = bow_store_fault(c, kfs[s], cur[s], "lmono_keyframes_detect_loop")) return rc;
        if (kfs[s]->voc != kfs[0]->voc) { c->err = "lmono_keyframes_detect_loop_batch: the stores must share one vocabulary"; return LMONO_EINVAL; }
    }
    std::vector<BowResult> res((size_t)n);
    std::vector<int> max_id((size_t)n);
    for (int s = 0; s < n; s++) max_id[(size_t)s] = (int)std::max<long long>((long long)cur[s] - loop_search_gap, INT_MIN);
    if (int rc = bow_query(c, n, kfs, cur, max_id.data(), 4, res.data())) return rc;
    for (int s = 0; s < n; s++) {
        const BowResult &r = res[(size_t)s];
        if (loop_index_out) loop_index_out[s] = bow_detect_rule(cur[s], loop_search_gap, r.n, r.id, r.score);
        if (n_out) n_out[s] = r.n;
        for (int i = 0; i < r.n; i++) { if (id_h) id_h[4 * (size_t)s + i] = r.id[i]; if (score_h) score_h[4 * (size_t)s + i] = r.score[i]; }
    }
    return LMONO_OK;
}

extern "C" int lmono_keyframes_detect_loop(lmono_ctx *c, lmono_keyframes *k, int cur, int loop_search_gap, int *loop_index_out, int *n_out, int32_t *id_h, double *score_h)
{
    if (!c || !k || k->ctx != c) return LMONO_EINVAL;
    return lmono_keyframes_detect_loop_batch(c, 1, &k, &cur, loop_search_gap, loop_index_out, n_out, id_h, score_h);
}
