// ba_abi.hip -- C ABI of the BA factors and the window solve: ba.hip, ba_solve.hip (included by lmono_hip.hip after lmono_ctx is defined)
#pragma once
// ---- BA factors -------------------------------------------------------------------------------------------------
extern "C" int lmono_factor_eval_blocks_d(lmono_ctx *c, int kind, int count, const double *params_d, const double *consts_d,
                                          const double *info_d, double *r_d, double *J_d, const unsigned char *block_mask_d)
{
    if (!c || kind < 0 || kind > 3 || count < 0 || !params_d || !consts_d || !info_d || !r_d) return LMONO_EINVAL;
    if (count == 0) return LMONO_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_factor_eval, dim3((count + 63) / 64), dim3(64), 0, c->stream, kind, count, params_d, consts_d, info_d, r_d, J_d, block_mask_d);
    return check_launch(c, "k_factor_eval");
}

extern "C" int lmono_factor_eval_d(lmono_ctx *c, int kind, int count, const double *params_d, const double *consts_d,
                                   const double *info_d, double *r_d, double *J_d)
{
    return lmono_factor_eval_blocks_d(c, kind, count, params_d, consts_d, info_d, r_d, J_d, nullptr);
}

extern "C" int lmono_factor_eval_blocks(lmono_ctx *c, int kind, int count, const double *params_h, const double *consts_h,
                                        const double *info_h, double *r_h, double *J_h, const unsigned char *block_mask_h)
{
    if (!c || kind < 0 || kind > 3 || count < 0 || !params_h || !consts_h || !info_h || !r_h) return LMONO_EINVAL;
    if (count == 0) return LMONO_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const FactorDims d = factor_dims(kind);
    double *p = nullptr, *cn = nullptr, *inf = nullptr, *r = nullptr, *J = nullptr;
    unsigned char *mk = nullptr;
    DevOwner mem;               // the call's six buffers: freed on every return
    // every failure below answers LMONO_ENODEV with "<the HIP call>: <its error>"
    auto bad = [&](hipError_t e, const char *call) { if (e != hipSuccess) c->err = std::string(call) + ": " + hipGetErrorString(e); return e != hipSuccess; };
    auto no_mem = [&](bool allocated, const char *call) { return bad(allocated ? hipSuccess : hipGetLastError(), call); };
    if (no_mem(mem.alloc(p, (size_t)d.np * count), "hipMalloc((void **)&p, sizeof(double) * d.np * count)") ||
        no_mem(mem.alloc(cn, (size_t)d.nc * count), "hipMalloc((void **)&cn, sizeof(double) * d.nc * count)") ||
        no_mem(mem.alloc(inf, (size_t)d.ni), "hipMalloc((void **)&inf, sizeof(double) * d.ni)") ||
        no_mem(mem.alloc(r, (size_t)d.nr * count), "hipMalloc((void **)&r, sizeof(double) * d.nr * count)") ||
        (J_h && no_mem(mem.alloc(J, (size_t)d.nj * count), "hipMalloc((void **)&J, sizeof(double) * d.nj * count)"))) return LMONO_ENODEV;
    // a mask: blocks the caller did not ask for keep the caller's bytes, so J starts from the caller's J
    if (J_h && block_mask_h &&
        (no_mem(mem.alloc(mk, (size_t)count), "hipMalloc((void **)&mk, (size_t)count)") ||
         bad(hipMemcpy(mk, block_mask_h, (size_t)count, hipMemcpyHostToDevice), "hipMemcpy(mk, block_mask_h, (size_t)count, hipMemcpyHostToDevice)") ||
         bad(hipMemcpy(J, J_h, sizeof(double) * d.nj * count, hipMemcpyHostToDevice), "hipMemcpy(J, J_h, sizeof(double) * d.nj * count, hipMemcpyHostToDevice)"))) return LMONO_ENODEV;
    if (bad(hipMemcpy(p, params_h, sizeof(double) * d.np * count, hipMemcpyHostToDevice), "hipMemcpy(p, params_h, sizeof(double) * d.np * count, hipMemcpyHostToDevice)") ||
        bad(hipMemcpy(cn, consts_h, sizeof(double) * d.nc * count, hipMemcpyHostToDevice), "hipMemcpy(cn, consts_h, sizeof(double) * d.nc * count, hipMemcpyHostToDevice)") ||
        bad(hipMemcpy(inf, info_h, sizeof(double) * d.ni, hipMemcpyHostToDevice), "hipMemcpy(inf, info_h, sizeof(double) * d.ni, hipMemcpyHostToDevice)")) return LMONO_ENODEV;
    if (int rc = lmono_factor_eval_blocks_d(c, kind, count, p, cn, inf, r, J, mk)) return rc;
    if (bad(hipStreamSynchronize(c->stream), "hipStreamSynchronize(c->stream)") ||
        bad(hipMemcpy(r_h, r, sizeof(double) * d.nr * count, hipMemcpyDeviceToHost), "hipMemcpy(r_h, r, sizeof(double) * d.nr * count, hipMemcpyDeviceToHost)") ||
        (J_h && bad(hipMemcpy(J_h, J, sizeof(double) * d.nj * count, hipMemcpyDeviceToHost), "hipMemcpy(J_h, J, sizeof(double) * d.nj * count, hipMemcpyDeviceToHost)"))) return LMONO_ENODEV;
    return LMONO_OK;
}

extern "C" int lmono_factor_eval(lmono_ctx *c, int kind, int count, const double *params_h, const double *consts_h,
                                 const double *info_h, double *r_h, double *J_h)
{
    return lmono_factor_eval_blocks(c, kind, count, params_h, consts_h, info_h, r_h, J_h, nullptr);
}

// ---- BA window solve ---------------------------------------------------------------------------------------------
struct lmono_ba_batch {
    lmono_ctx *ctx = nullptr;
    // ONE device allocation holds every array of the problem: [uploaded arrays | scratch that starts zeroed], each 256-B aligned, laid out
    // anew by every ba_fill; ONE pinned host buffer stages the uploaded part.  A frame loop (lmono_ba_batch_update per frame) therefore costs
    // one H2D copy and one memset per frame instead of 21 pageable copies and 6 memsets, and allocates nothing in steady state.
    char *blob = nullptr; size_t blob_cap = 0;
    char *stage = nullptr; size_t stage_cap = 0;
    BaBatch v{};
    int n_windows = 0, total_feat = 0, total_obs = 0;
    int cluster = 1;            // workgroups per window of the last fill (the scratch is sized for it)
    bool big = false;           // a window of the last fill holds more than kBaLdsFeat features: the kBig kernels (per-feature vectors in an L2 scratch)
    bool flags_clean = false;   // the cluster's flag words and the failure flag are zero (a fill zeroes them; a solve dirties them)
    double *poses0 = nullptr, *ex0 = nullptr, *invd0 = nullptr;   // initial state for lmono_ba_batch_reset
    // the state (poses | ex | inverse depths: neighbours in the blob) as it was before the last CLUSTER solve, and that solve's iteration cap: a cluster whose
    // workgroups were not all resident gives up (bounded polls) and lmono_ba_batch_read runs the solve again with one workgroup per window from here
    // -- same bytes by construction
    char *pre = nullptr; size_t pre_bytes = 0;
    int retries = 0;            // cluster solves that had to be run again (diagnosis; LMONO_BA_TEST_FAIL exercises the path)
};

// the arrays of one ba_fill: laid out first (add), then staged / placed in one go (commit)
struct BaPack {
    struct Item { void **dst; const void *src; size_t bytes, off; };
    std::vector<Item> items;
    size_t up = 0, zero = 0;
    template <typename T> void add(T *&dst, const T *src, size_t count)
    {
        const size_t bytes = (count > 0 ? count : 1) * sizeof(T), al = (bytes + 255) & ~(size_t)255;
        items.push_back({ (void **)&dst, (const void *)src, src ? count * sizeof(T) : 0, src ? up : zero });
        (src ? up : zero) += al;
    }
    int commit(lmono_ctx *c, lmono_ba_batch *b)
    {
        const size_t total = up + zero;
        if (b->blob_cap < total) {
            if (b->blob) HIP_TRY(c, hipFree(b->blob));
            b->blob = nullptr; b->blob_cap = 0;
            const size_t cap = total + total / 2;
            HIP_TRY(c, hipMalloc((void **)&b->blob, cap));
            b->blob_cap = cap;
        }
        if (b->stage_cap < up) {
            if (b->stage) HIP_TRY(c, hipHostFree(b->stage));
            b->stage = nullptr; b->stage_cap = 0;
            const size_t cap = up + up / 2;
            HIP_TRY(c, hipHostMalloc((void **)&b->stage, cap, hipHostMallocDefault));
            b->stage_cap = cap;
        }
        for (const Item &it : items) {
            if (it.src) { memcpy(b->stage + it.off, it.src, it.bytes); *it.dst = b->blob + it.off; }
            else *it.dst = b->blob + up + it.off;
        }
        if (up) HIP_TRY(c, hipMemcpyAsync(b->blob, b->stage, up, hipMemcpyHostToDevice, c->stream));
        if (zero) HIP_TRY(c, hipMemsetAsync(b->blob + up, 0, zero, c->stream));
        b->flags_clean = true;
        return LMONO_OK;
    }
};

extern "C" void lmono_ba_batch_destroy(lmono_ba_batch *b)
{
    if (!b) return;
    if (b->retries > 0 && getenv("LMONO_BA_REPORT_RETRIES")) fprintf(stderr, "[lmono] lmono_ba_batch: %d cluster solve(s) gave up and were run again with one workgroup per window\n", b->retries);
    if (b->ctx) (void)hipStreamSynchronize(b->ctx->stream);
    if (b->blob) (void)hipFree(b->blob);
    if (b->stage) (void)hipHostFree(b->stage);
    delete b;
}

// validate the descriptor, build the pair-ordered tables and (re)load every device array of the batch
static int ba_fill(lmono_ctx *c, lmono_ba_batch *b, const lmono_ba_desc *d)
{
    if (!d || d->n_windows <= 0 || !d->feat_off || !d->obs_off || !d->flags || !d->poses || !d->ex) { c->err = "lmono_ba_batch: bad descriptor"; return LMONO_EINVAL; }
    if (!d->laser_info || !d->mono_info || !d->prior_w || !d->laser_consts || !d->prior_T || (d->feat_off[d->n_windows] > 0 && !d->inv_depth)) { c->err = "lmono_ba_batch_create: a descriptor array is NULL"; return LMONO_EINVAL; }
    if (d->obs_off[d->n_windows] > 0 && (!d->obs_feat || !d->obs_i || !d->obs_j || !d->obs_pts)) { c->err = "lmono_ba_batch_create: observation arrays are NULL"; return LMONO_EINVAL; }
    HIP_TRY(c, hipSetDevice(c->device));
    const int W = d->n_windows;
    const int TF = d->feat_off[W], TO = d->obs_off[W];
    for (int w = 0; w < W; w++) {
        if (d->feat_off[w + 1] - d->feat_off[w] > kBaMaxFeat) { c->err = "lmono_ba_batch_create: more than LMONO_BA_MAX_FEATURES (" + std::to_string(kBaMaxFeat) + ") features in a window"; return LMONO_ECAPACITY; }
        if (d->flags[4 * w] < 2 || d->flags[4 * w] > kBaMaxPoses) { c->err = "lmono_ba_batch_create: n_poses must be 2..11"; return LMONO_EINVAL; }
    }
    // first observation of every feature: observations must be grouped by (window, feature) in ascending order
    std::vector<int> fo((size_t)TF + 1, 0);
    {
        int o = 0;
        for (int w = 0; w < W; w++) {
            const int f0 = d->feat_off[w], f1 = d->feat_off[w + 1], oe = d->obs_off[w + 1];
            o = d->obs_off[w];
            for (int f = f0; f < f1; f++) {
                fo[f] = o;
                while (o < oe && d->obs_feat[o] == f - f0) {
                    const int np = d->flags[4 * w];
                    if (d->obs_i[o] < 0 || d->obs_i[o] >= np || d->obs_j[o] < 0 || d->obs_j[o] >= np || d->obs_i[o] == d->obs_j[o]) { c->err = "lmono_ba_batch_create: bad observation frame"; return LMONO_EINVAL; }
                    o++;
                }
            }
            if (o != oe) { c->err = "lmono_ba_batch_create: observations are not grouped by feature"; return LMONO_EINVAL; }
        }
        fo[TF] = TO;
    }
    // frame pairs of every window (descending observation count: the waves take them from a work counter) and the
    // pair-ordered observation list
    std::vector<int> pair_off((size_t)W + 1, 0), pair_ij, pair_slot, pobs_off((size_t)W + 1, 0), slot_info, anchor((size_t)TF, -1);
    std::vector<double> slot_pts;
    std::vector<unsigned short> seg_tab;            // segments (<= 16 slots of one pair): pair (window-local) | index inside the pair << 7
    std::vector<int> seg_off((size_t)W + 1, 0), pair_seg, n_multi((size_t)W, 0);
    std::vector<int> slot_obs;                      // the observation (host order) behind every slot: its scratch record is indexed by observation,
                                                    // so a feature's records are contiguous for the per-feature sums of k_ba_solve
    slot_info.reserve((size_t)TO); slot_obs.reserve((size_t)TO); slot_pts.reserve((size_t)TO * 4); seg_tab.reserve((size_t)TO / 8 + (size_t)W * 16);
    pair_ij.reserve((size_t)W * 64); pair_slot.reserve((size_t)W * 65); pair_seg.reserve((size_t)W * 65);
    for (int w = 0; w < W; w++) {
        pair_off[w] = (int)pair_ij.size(); pobs_off[w] = (int)slot_info.size(); seg_off[w] = (int)seg_tab.size();
        const int f0 = d->feat_off[w], f1 = d->feat_off[w + 1];
        for (int f = f0; f < f1; f++) if (fo[f + 1] > fo[f]) anchor[f] = d->obs_i[fo[f]];
        if (d->flags[4 * w + 3]) {   // use_mono == 0: the projection factors are not part of the problem
            // counting sort of the window's observations by frame pair (ascending observation index inside a pair), pairs by (observer j, anchor i) ascending
            // (since round 6; the order of the sums, so part of the result's bits.  Rounds 4-5 sorted by descending size for the waves' work counter, which
            // the 16-slot segments made pointless) -- no per-window allocations: a lock-step batch of Estimators fills hundreds of windows per frame
            constexpr int kKeys = kBaMaxPoses * kBaMaxPoses;
            int cnt[kKeys], base[kKeys], order[kKeys], local_of[kKeys], n_keys = 0;
            for (int key = 0; key < kKeys; key++) cnt[key] = 0;
            const int o0w = d->obs_off[w], o1w = d->obs_off[w + 1];
            for (int o = o0w; o < o1w; o++) cnt[d->obs_i[o] * kBaMaxPoses + d->obs_j[o]]++;
            for (int j = 0; j < kBaMaxPoses; j++) for (int i = 0; i < kBaMaxPoses; i++) { const int key = i * kBaMaxPoses + j; if (cnt[key] > 0) order[n_keys++] = key; }
            const size_t slot0 = slot_info.size();
            int run = 0;
            for (int local = 0; local < n_keys; local++) {
                const int key = order[local];
                local_of[key] = local; base[key] = run;
                pair_ij.push_back((key / kBaMaxPoses) | ((key % kBaMaxPoses) << 8));
                pair_slot.push_back(run);
                pair_seg.push_back((int)seg_tab.size() - seg_off[w]);
                const int nseg = (cnt[key] + kBaSeg - 1) / kBaSeg;
                for (int sidx = 0; sidx < nseg; sidx++) seg_tab.push_back((unsigned short)(local | (sidx << 7)));
                if (nseg > 1) n_multi[w]++;
                run += cnt[key];
            }
            slot_obs.resize(slot0 + (size_t)run); slot_info.resize(slot0 + (size_t)run); slot_pts.resize((slot0 + (size_t)run) * 4);
            for (int o = o0w; o < o1w; o++) {
                const int key = d->obs_i[o] * kBaMaxPoses + d->obs_j[o];
                const size_t sl = slot0 + (size_t)base[key]++;
                slot_obs[sl] = o;
                slot_info[sl] = d->obs_feat[o] | (local_of[key] << 16);
                memcpy(&slot_pts[sl * 4], &d->obs_pts[(size_t)o * 4], 4 * sizeof(double));
            }
        }
        pair_slot.push_back((int)slot_info.size() - pobs_off[w]);   // n_pairs + 1 entries per window
        pair_seg.push_back((int)seg_tab.size() - seg_off[w]);
    }
    pair_off[W] = (int)pair_ij.size(); pobs_off[W] = (int)slot_info.size(); seg_off[W] = (int)seg_tab.size();
    b->ctx = c; b->n_windows = W; b->total_feat = TF; b->total_obs = TO;
    BaBatch &v = b->v;
    v.n_windows = W; v.max_iter = 30;
    double info[42];
    memcpy(info, d->laser_info, 36 * sizeof(double)); memcpy(info + 36, d->mono_info, 4 * sizeof(double)); memcpy(info + 40, d->prior_w, 2 * sizeof(double));
    int *feat_off = nullptr, *obs_off = nullptr, *flags = nullptr, *anch = nullptr, *poff = nullptr, *pij = nullptr, *psoff = nullptr, *sinfo_d = nullptr, *pslot_d = nullptr;
    int *fobs_d = nullptr, *oslot_d = nullptr, *segoff_d = nullptr, *pseg_d = nullptr, *nmulti_d = nullptr;
    unsigned short *segtab_d = nullptr;
    const unsigned short uzero = 0;
    double *spts_d = nullptr, *laser = nullptr, *prior = nullptr, *infod = nullptr;
    const int izero = 0; const double dzero = 0.0;       // a present (non-NULL) source for arrays that may be empty
    BaPack pk;
    pk.add(feat_off, d->feat_off, (size_t)W + 1); pk.add(obs_off, d->obs_off, (size_t)W + 1);
    std::vector<double> zsum((size_t)W * 6, 0.0);
    pk.add(flags, d->flags, (size_t)W * 4);
    pk.add(v.fail, &izero, (size_t)1); pk.add(v.summary, (const double *)zsum.data(), (size_t)W * 6);        // [failure flag | summaries | poses | ex | inverse depths]: the results, one read-back
    pk.add(v.poses, d->poses, (size_t)W * kBaMaxPoses * 7);
    pk.add(v.ex, d->ex, (size_t)W * 7); pk.add(v.inv_depth, TF ? d->inv_depth : &dzero, (size_t)TF);
    pk.add(anch, TF ? anchor.data() : &izero, (size_t)TF);
    pk.add(poff, pair_off.data(), (size_t)W + 1); pk.add(pij, pair_ij.empty() ? &izero : pair_ij.data(), pair_ij.size());
    pk.add(psoff, pobs_off.data(), (size_t)W + 1); pk.add(sinfo_d, slot_info.empty() ? &izero : slot_info.data(), slot_info.size());
    pk.add(spts_d, slot_pts.empty() ? &dzero : slot_pts.data(), slot_pts.size()); pk.add(pslot_d, pair_slot.data(), pair_slot.size());
    pk.add(laser, d->laser_consts, (size_t)W * 10 * 24); pk.add(prior, d->prior_T, (size_t)W * 16);
    pk.add(infod, (const double *)info, (size_t)42);
    pk.add(b->poses0, d->poses, (size_t)W * kBaMaxPoses * 7); pk.add(b->ex0, d->ex, (size_t)W * 7);
    pk.add(b->invd0, TF ? d->inv_depth : &dzero, (size_t)TF);
    pk.add(fobs_d, (const int *)fo.data(), (size_t)TF + 1); pk.add(oslot_d, slot_obs.empty() ? &izero : slot_obs.data(), slot_obs.size());
    pk.add(segoff_d, (const int *)seg_off.data(), (size_t)W + 1); pk.add(pseg_d, (const int *)pair_seg.data(), pair_seg.size());
    pk.add(nmulti_d, (const int *)n_multi.data(), (size_t)W); pk.add(segtab_d, seg_tab.empty() ? &uzero : seg_tab.data(), seg_tab.size());
    pk.add(v.obsc, (const double *)nullptr, (size_t)TO * kBaObsRec);
    b->big = false;
    for (int w = 0; w < W; w++) if (d->feat_off[w + 1] - d->feat_off[w] > kBaLdsFeat) b->big = true;
    v.feat_cap = b->big ? kBaMaxFeat : kBaLdsFeat;
    pk.add(v.hpd, (const double *)nullptr, (size_t)W * v.feat_cap * kBaPS);
    pk.add(v.bigv, (const double *)nullptr, b->big ? (size_t)W * 8 * kBaMaxFeat : (size_t)1);
    // workgroups per window: several when the batch leaves most of the chip idle (every workgroup of a window must be resident while it polls: at most
    // half the CUs).  LMONO_BA_CLUSTER = 1 / 2 / 4 forces it (measurement switch); the results do not depend on it, bit for bit.
    {
        static const int env = [] { const char *e = getenv("LMONO_BA_CLUSTER"); return e ? atoi(e) : 0; }();        // measurement switch
        const int forced = c->opt[LMONO_OPT_BA_CLUSTER] > 0 ? c->opt[LMONO_OPT_BA_CLUSTER] : env;
        int K = forced > 0 ? forced : kBaMaxK;
        // (a window of few segments gains nothing from the last doubling and pays its hand-offs: the Estimator's own windows, ~45 segments, run 0.5 % faster
        // at 4 than at 8, the 110-segment bench window 5 % slower; the bytes are the same either way)
        if (forced <= 0 && (int)seg_tab.size() < 64 * W) K = 4;
        if (K > kBaMaxK) K = kBaMaxK;
        if (K == 3) K = 2; else if (K > 4 && K < 8) K = 4;
        while (K > 1 && ((W + 7) / 8) * 8 * K > c->cluster_budget) K >>= 1;      // (256 CUs: 128 workgroups -- 8 for up to 16 windows ... 1 above 64)
        b->cluster = K;
    }
    pk.add(v.pairdat, (const double *)nullptr, (size_t)b->cluster * pair_ij.size() * kBaPairRec);
    pk.add(v.mbox, (const double *)nullptr, (size_t)W * kBaMbox);
    pk.add(v.bar, (const unsigned int *)nullptr, (size_t)W * kBaBar);
    v.n_pairs_total = (int)pair_ij.size();
    pk.add(v.pairH, (const double *)nullptr, (seg_tab.size() + pair_ij.size() + (size_t)W) * kBaPairTile);
    pk.add(v.gprog, (const int *)nullptr, (size_t)W * kBaGprog);
    pk.add(v.cpart, (const double *)nullptr, seg_tab.size());
    pk.add(v.cand, (const double *)nullptr, (size_t)W * v.feat_cap);
    {
        auto al = [](size_t bytes) { return ((bytes ? bytes : 8) + 255) & ~(size_t)255; };
        b->pre_bytes = al(sizeof(double) * (size_t)W * kBaMaxPoses * 7) + al(sizeof(double) * (size_t)W * 7) + al(sizeof(double) * (size_t)TF);
        pk.add(b->pre, (const char *)nullptr, b->pre_bytes);
    }
    // everything is staged in the batch's pinned buffer: the vectors above may go, and nothing waits here
    { const int rc = pk.commit(c, b); if (rc) { c->err = "lmono_ba_batch_create: device allocation / upload failed"; return LMONO_ENOMEM; } }
    v.feat_off = feat_off; v.obs_off = obs_off; v.flags = flags; v.feat_anchor = anch;
    v.pair_off = poff; v.pair_ij = pij; v.pobs_off = psoff; v.slot_info = sinfo_d; v.slot_pts = spts_d; v.pair_slot = pslot_d;
    v.laser_consts = laser; v.prior_T = prior; v.info = infod;
    v.feat_obs_off = fobs_d; v.slot_obs = oslot_d;
    v.seg_off = segoff_d; v.seg_tab = segtab_d; v.pair_seg = pseg_d; v.n_multi = nmulti_d;
    v.blob_lo = b->blob; v.blob_hi = b->blob + pk.up + pk.zero;      // (the arrays of THIS fill: what lies behind them in a larger, re-used allocation is out of bounds too)
    return LMONO_OK;
}

extern "C" lmono_ba_batch *lmono_ba_batch_create(lmono_ctx *c, const lmono_ba_desc *d)
{
    if (!c) return nullptr;
    lmono_ba_batch *b = new lmono_ba_batch();
    b->ctx = c;
    if (ba_fill(c, b, d) != LMONO_OK) { lmono_ba_batch_destroy(b); return nullptr; }
    return b;
}

// Load another set of windows into an existing batch (the Estimator's next frame): device arrays are reused where they are large
// enough, so a steady-state frame loop allocates nothing.  On error the batch holds no valid problem until the next update.
extern "C" int lmono_ba_batch_update(lmono_ctx *c, lmono_ba_batch *b, const lmono_ba_desc *d)
{
    if (!c || !b || b->ctx != c) return LMONO_EINVAL;
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // a solve of the previous problem may still read the arrays
    const int rc = ba_fill(c, b, d);
    if (rc != LMONO_OK) { b->n_windows = 0; b->total_feat = 0; b->total_obs = 0; }     // no problem: solve / reset / read refuse
    return rc;
}

static int ba_launch_single(lmono_ctx *c, lmono_ba_batch *b)
{
    if (b->big) hipLaunchKernelGGL((k_ba_solve<false, true>), dim3(b->n_windows), dim3(kBaT), 0, c->stream, b->v, 1, 0);
    else hipLaunchKernelGGL((k_ba_solve<false, false>), dim3(b->n_windows), dim3(kBaT), 0, c->stream, b->v, 1, 0);          // its LDS is static (g_ba_lds)
    return check_launch(c, "k_ba_solve");
}

extern "C" int lmono_ba_solve(lmono_ctx *c, lmono_ba_batch *b, int max_iterations)
{
    if (!c || !b || max_iterations < 0) return LMONO_EINVAL;
    if (b->n_windows <= 0) { c->err = "lmono_ba_solve: the batch holds no problem (failed update)"; return LMONO_EINVAL; }
    HIP_TRY(c, hipSetDevice(c->device));
    b->v.max_iter = max_iterations;
    if (b->cluster > 1) {
        // the flag words start at zero in every launch (the first solve after a fill finds them zeroed with the rest of the scratch)
        if (!b->flags_clean) {
            HIP_TRY(c, hipMemsetAsync(b->v.bar, 0, sizeof(unsigned int) * (size_t)b->n_windows * kBaBar, c->stream));
            HIP_TRY(c, hipMemsetAsync(b->v.fail, 0, sizeof(int), c->stream));
        }
        b->flags_clean = false;
        // the state this solve starts from, for the one-workgroup re-run of a cluster that was not resident (lmono_ba_batch_read)
        if ((const char *)(b->v.inv_depth + b->total_feat) - (const char *)b->v.poses <= (ptrdiff_t)b->pre_bytes && (const char *)b->v.ex > (const char *)b->v.poses)
            HIP_TRY(c, hipMemcpyAsync(b->pre, b->v.poses, (size_t)((const char *)(b->v.inv_depth + b->total_feat) - (const char *)b->v.poses), hipMemcpyDeviceToDevice, c->stream));
        static const int test_fail = [] { const char *e = getenv("LMONO_BA_TEST_FAIL"); return e ? atoi(e) : 0; }();   // test hook: the cluster gives up at its first poll
        if (test_fail) HIP_TRY(c, hipMemsetAsync(b->v.fail, 1, 1, c->stream));
        static const int spread = [] { const char *e = getenv("LMONO_BA_SPREAD"); return (e && atoi(e)) ? 1 : 0; }();      // test hook: a window's workgroups on different XCDs
        const dim3 grid(((b->n_windows + 7) / 8) * 8 * b->cluster);
        if (b->big) hipLaunchKernelGGL((k_ba_solve<true, true>), grid, dim3(kBaT), 0, c->stream, b->v, b->cluster, spread);
        else hipLaunchKernelGGL((k_ba_solve<true, false>), grid, dim3(kBaT), 0, c->stream, b->v, b->cluster, spread);
        return check_launch(c, "k_ba_solve");
    }
    return ba_launch_single(c, b);
}

// Diagnostic: the bounds-checked build's record (-DLMONO_BOUNDS, lmono_amd/csrc/ba_solve.hip ba_chk): out[0] accesses of k_ba_solve outside the batch's
// allocation since the library was loaded, out[1] source line of the first, out[2] its byte offset from the allocation's start, out[3] its block.
// The product build has no checks and answers LMONO_EINVAL.
extern "C" int lmono_debug_bounds(lmono_ctx *c, unsigned long long *out4)
{
    if (!c || !out4) return LMONO_EINVAL;
#ifdef LMONO_BOUNDS
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_ba_oob), 4 * sizeof(unsigned long long)));
    return LMONO_OK;
#else
    c->err = "lmono_debug_bounds: this build carries no bounds checks (build with -DLMONO_BOUNDS)";
    return LMONO_EINVAL;
#endif
}

extern "C" int lmono_ba_batch_reset(lmono_ctx *c, lmono_ba_batch *b)
{
    if (!c || !b) return LMONO_EINVAL;
    if (b->n_windows <= 0) { c->err = "lmono_ba_batch_reset: the batch holds no problem (failed update)"; return LMONO_EINVAL; }
    HIP_TRY(c, hipMemcpyAsync(b->v.poses, b->poses0, sizeof(double) * (size_t)b->n_windows * kBaMaxPoses * 7, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(b->v.ex, b->ex0, sizeof(double) * (size_t)b->n_windows * 7, hipMemcpyDeviceToDevice, c->stream));
    if (b->total_feat > 0) HIP_TRY(c, hipMemcpyAsync(b->v.inv_depth, b->invd0, sizeof(double) * (size_t)b->total_feat, hipMemcpyDeviceToDevice, c->stream));
    return LMONO_OK;
}

static int ba_read(lmono_ctx *c, lmono_ba_batch *b, double *poses_h, double *ex_h, double *inv_depth_h, double *summary_h, bool may_retry);
extern "C" int lmono_ba_batch_read(lmono_ctx *c, lmono_ba_batch *b, double *poses_h, double *ex_h, double *inv_depth_h, double *summary_h)
{
    return ba_read(c, b, poses_h, ex_h, inv_depth_h, summary_h, true);
}
static int ba_read(lmono_ctx *c, lmono_ba_batch *b, double *poses_h, double *ex_h, double *inv_depth_h, double *summary_h, bool may_retry)
{
    if (!c || !b) return LMONO_EINVAL;
    if (b->n_windows <= 0) { c->err = "lmono_ba_batch_read: the batch holds no problem (failed update)"; return LMONO_EINVAL; }
    // (failure flag | summaries | poses | ex | inverse depths) are neighbours in the batch's allocation: a small batch -- the Estimator's one window per
    // frame -- comes back as ONE copy into the batch's pinned staging buffer (free between an upload and the next) instead of five copies into pageable
    // memory, each of which the runtime stages and waits for on its own.
    const size_t w = (size_t)b->n_windows;
    const char *lo = (const char *)b->v.fail;
    const size_t bytes = (size_t)((const char *)(b->v.inv_depth + b->total_feat) - lo);
    int failed = 0;
    if ((const char *)b->v.summary > lo && (const char *)b->v.poses > (const char *)b->v.summary && (const char *)b->v.ex > (const char *)b->v.poses &&
        (const char *)b->v.inv_depth > (const char *)b->v.ex && bytes + 256 <= b->stage_cap && bytes <= ((size_t)256 << 10)) {
        char *sa = b->stage;
        HIP_TRY(c, hipMemcpyAsync(sa, lo, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));      // stream-ordered behind the solve; nothing goes through the null stream
        if (poses_h) memcpy(poses_h, sa + ((const char *)b->v.poses - lo), sizeof(double) * w * kBaMaxPoses * 7);
        if (ex_h) memcpy(ex_h, sa + ((const char *)b->v.ex - lo), sizeof(double) * w * 7);
        if (inv_depth_h && b->total_feat > 0) memcpy(inv_depth_h, sa + ((const char *)b->v.inv_depth - lo), sizeof(double) * (size_t)b->total_feat);
        if (summary_h) memcpy(summary_h, sa + ((const char *)b->v.summary - lo), sizeof(double) * w * 6);
        if (b->cluster > 1) memcpy(&failed, sa, sizeof(int));
    } else {
        if (poses_h) HIP_TRY(c, hipMemcpyAsync(poses_h, b->v.poses, sizeof(double) * w * kBaMaxPoses * 7, hipMemcpyDeviceToHost, c->stream));
        if (ex_h) HIP_TRY(c, hipMemcpyAsync(ex_h, b->v.ex, sizeof(double) * w * 7, hipMemcpyDeviceToHost, c->stream));
        if (inv_depth_h && b->total_feat > 0) HIP_TRY(c, hipMemcpyAsync(inv_depth_h, b->v.inv_depth, sizeof(double) * (size_t)b->total_feat, hipMemcpyDeviceToHost, c->stream));
        if (summary_h) HIP_TRY(c, hipMemcpyAsync(summary_h, b->v.summary, sizeof(double) * w * 6, hipMemcpyDeviceToHost, c->stream));
        if (b->cluster > 1) HIP_TRY(c, hipMemcpyAsync(&failed, b->v.fail, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (failed && may_retry && b->pre) {
        // A workgroup of some window's cluster did not arrive within the poll bound (a CU mask, a partition, another process's resident workgroups: the
        // residency budget is a guess about a card this context does not own).  Every window of the launch may have stopped early, so the whole solve runs
        // again from the state it started from with ONE workgroup per window, which needs nobody resident but itself -- the same bytes (the sums are formed
        // per segment in segment order whatever K is).
        b->retries++;
        const size_t range = (size_t)((const char *)(b->v.inv_depth + b->total_feat) - (const char *)b->v.poses);
        HIP_TRY(c, hipMemcpyAsync(b->v.poses, b->pre, range, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(b->v.fail, 0, sizeof(int), c->stream));
        const int rc = ba_launch_single(c, b);
        if (rc) return rc;
        return ba_read(c, b, poses_h, ex_h, inv_depth_h, summary_h, false);
    }
    if (failed) { c->err = "k_ba_solve: a workgroup of a window's cluster did not arrive (not all resident?): the solve is void"; return LMONO_ENODEV; }
    return LMONO_OK;
}
