// lmono_amd/csrc/lmono_hip.hip -- C ABI (include/lmono_hip.h) over the gfx950 kernels.  Single translation unit: the kernel files are included here, in one
// fixed order, and the ABI of each subsystem (*_abi.hip, at the end) behind lmono_ctx, so that one `hipcc -shared` produces liblmono_hip.so.
#include "line_index.hip"
#include "frontend.hip"
#include "trust_region.hpp"
#include "odometry.hip"
#include "corr_flat.hip"
#include "mapping.hip"
#include "ba.hip"
#include "ba_solve.hip"
#include "feat.hip"
#include "marg.hip"

#include <string>
#include <vector>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <atomic>
#include <functional>
#include <memory>
#include <chrono>
#include <algorithm>
#include <cstdio>
#include <cstring>


using namespace lmono;

struct EvSet { hipEvent_t e[10]; bool reg = false, odom = false; std::vector<hipEvent_t> kev; int n_kev = 0; };  // kev: (begin, mid, end) per odometry launch pair

#include "host_workers.hpp"
#include "dev_owner.hpp"

// per-thread tables of lmono_mapper_process_batch's update plan (indexed by cube: 21 x 21 x 11)
struct MapPlanScratch {
    struct Run { int ind, at, len; };
    std::vector<char> is_valid; std::vector<int> add, fill, cand; std::vector<int64_t> cat_off; std::vector<Run> runs;
    MapPlanScratch() : is_valid((size_t)lmono::kMdCubes, 0), add((size_t)lmono::kMdCubes, 0), fill((size_t)lmono::kMdCubes, 0), cat_off((size_t)lmono::kMdCubes, -1) {}
};

struct lmono_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::vector<EvSet> sets;   // one event set per scanreg/odometry call since the last lmono_timing_reset
    int n_sets = 0;
    hipEvent_t *ev = nullptr;  // events of the current call
    int opt[LMONO_OPT_COUNT] = { 3, 0, 4, -1, 1000, 0, 0 };   // (LMONO_OPT_LEAD_SEED: 0 until measured)   // LMONO_OPT_CORR_TILE: 3 = flattened sweeps (default, needs no hash grid), 0 = 32-lane groups on the hash grid (diagnostic build)
    hipStream_t gstream[8] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };   // streams of the odometry's chain groups (LMONO_OPT_ODOM_STREAMS > 1)
    hipEvent_t gev[9] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    unsigned long long *stats_d = nullptr;   // [0] feature points deferred by the tile search since the last lmono_timing_reset
    hipStream_t copy_stream = nullptr;       // H2D staging of lmono_batch_stage_h (runs beside the compute stream)
    hipStream_t own_stream = nullptr;        // lmono_use_own_stream: a stream of the library's that this context runs on
    bool odom_prio = false, many_queues = false;     // measurement switches read from the environment at creation (LMONO_ODOM_STREAM_PRIORITY, GPU_MAX_HW_QUEUES >= 8)
    int lm_planes = kLmPlanesDefault;                // k_lm_solve<planes>: 16-B planes of a staged block kept in LDS (measurement switch LMONO_LM_LDS_PLANES = 4 or 0 at creation)
    // scratch arena of the small host-array entry points (triangulate, outlier scores, marginalise ...): chunks are allocated once and
    // reused by every later call -- no hipMalloc / hipFree (both synchronise the device) in a steady-state frame loop
    struct Chunk { char *base; size_t cap; };
    std::vector<Chunk> arena;
    size_t arena_chunk = 0, arena_off = 0;
    int n_cu = 0;                            // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    int map_budget = 0;
    int cluster_budget = 0;                  // workgroups a cluster kernel (k_ba_solve<kCl>, k_map_solve) may keep resident while they poll each other: half the CUs
    char *stage = nullptr;                   // pinned staging of DevBuf's small uploads (stage_all: every buffer ever allocated, freed with the context)
    size_t stage_cap = 0;
    std::vector<void *> stage_all;
    std::vector<MapPlanScratch> plan_scratch;
    std::unique_ptr<HostWorkers> workers;    // created by the first batched call that has per-stream host work for them (LMONO_LIB_THREADS, default min(8, cores))

    hipEvent_t *next_set()
    {
        constexpr int kMaxSets = 1024;
        if (n_sets == (int)sets.size()) {
            if (n_sets >= kMaxSets) { sets[n_sets - 1].reg = sets[n_sets - 1].odom = false; return sets[n_sets - 1].e; }
            EvSet s;
            for (auto &e : s.e) if (hipEventCreate(&e) != hipSuccess) return nullptr;
            sets.push_back(s);
        }
        sets[n_sets].reg = sets[n_sets].odom = false;
        sets[n_sets].n_kev = 0;
        return sets[n_sets++].e;
    }
};

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                  \
            return e_ == hipErrorOutOfMemory ? LMONO_ENOMEM : LMONO_ENODEV;                  \
        }                                                                                    \
    } while (0)

static int check_launch(lmono_ctx *c, const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { c->err = std::string(what) + ": " + hipGetErrorString(e); return LMONO_ENODEV; }
    return LMONO_OK;
}

// ---- scratch arena and staged transfers of the host-array entry points (per-feature kernels, marginalisation, map refine, voxel filter)
namespace {
// Scratch of one ABI call, carved from the context's arena (released when the scope ends; the chunks stay).  Uploads are asynchronous on
// the context stream: nothing here touches the null stream or synchronises the device, so two contexts on two host threads overlap.
// Round 4: small uploads are STAGED -- copied into the context's pinned staging buffer at the same spacing as their device allocations and sent by
// ready() as one copy per run of adjacent allocations (the per-feature calls of a frame made ~25 separate pageable uploads, each a staged, host-blocking
// copy of its own).  Every user calls ready() behind its last up() and before its first launch.  A call's staged bytes are consumed before the call
// returns (every call ends waiting for its results), so the next call may overwrite them.
struct DevBuf {
    lmono_ctx *c;
    size_t chunk0, off0;
    bool used = false;
    static constexpr size_t kStageMax = (size_t)256 << 10;      // larger uploads (clouds) go directly
    char *run_dst = nullptr;         // device address of the pending run's first byte
    size_t run_at = 0, run_bytes = 0, stage_used = 0;
    explicit DevBuf(lmono_ctx *c_) : c(c_), chunk0(c_ ? c_->arena_chunk : 0), off0(c_ ? c_->arena_off : 0) {}
    bool send_run()
    {
        if (run_bytes == 0) return true;
        const bool sent = hipMemcpyAsync(run_dst, c->stage + run_at, run_bytes, hipMemcpyHostToDevice, c->stream) == hipSuccess;
        run_dst = nullptr; run_bytes = 0;
        return sent;
    }
    // every staged upload is on its way (call once, behind the last up() and before the first launch)
    void ready(bool &ok) { if (c && !send_run()) ok = false; }
    // Results come back the same way (round 5): small read-backs are queued into the pinned staging buffer -- device-adjacent ones as ONE copy -- and
    // handed to the caller's (pageable) arrays by fetch(), which waits for the stream once.  A copy into pageable memory is staged by the runtime on
    // its own and waited for one by one: ~20 us each in the Estimator's frame loop, four of them per frame.
    struct Pending { char *dst; size_t at, bytes; };
    std::vector<Pending> downs;
    const char *drun_src = nullptr; size_t drun_at = 0, drun_bytes = 0;
    bool flush_down()
    {
        if (drun_bytes == 0) return true;
        const bool sent = hipMemcpyAsync(c->stage + drun_at, drun_src, drun_bytes, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        drun_src = nullptr; drun_bytes = 0;
        return sent;
    }
    bool down(void *dst, const void *src, size_t bytes)
    {
        const size_t al = (bytes + 255) & ~(size_t)255;
        if (!c->stage || bytes > kStageMax || stage_used + al > c->stage_cap)
            return flush_down() && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        if (drun_bytes > 0 && (const char *)src != drun_src + drun_bytes && !flush_down()) return false;
        if (drun_bytes == 0) { drun_src = (const char *)src; drun_at = stage_used; }
        downs.push_back({ (char *)dst, stage_used, bytes });
        stage_used += al; drun_bytes += al;
        return true;
    }
    // every queued read-back is in the caller's arrays (waits for the stream)
    bool fetch()
    {
        if (!flush_down() || hipStreamSynchronize(c->stream) != hipSuccess) return false;
        for (const Pending &p : downs) memcpy(p.dst, c->stage + p.at, p.bytes);
        downs.clear();
        return true;
    }
    // the scratch goes back to the arena only once nothing queued on the stream can still touch it (a no-op wait on the normal path,
    // where the call has already waited for its results; it matters on the early error returns)
    ~DevBuf() { if (c) { if (used) (void)hipStreamSynchronize(c->stream); c->arena_chunk = chunk0; c->arena_off = off0; } }
    template <typename T> T *up(const T *src, size_t n, bool &ok)
    {
        if (!ok || !c) { ok = false; return nullptr; }
        used = true;
        const size_t bytes = (((n > 0 ? n : 1) * sizeof(T)) + 255) & ~(size_t)255;
        while (c->arena_chunk < c->arena.size() && c->arena_off + bytes > c->arena[c->arena_chunk].cap) { c->arena_chunk++; c->arena_off = 0; }
        if (c->arena_chunk == c->arena.size()) {
            size_t cap = c->arena.empty() ? (size_t)1 << 20 : 2 * c->arena.back().cap;
            while (cap < bytes) cap <<= 1;
            void *q = nullptr;
            if (hipMalloc(&q, cap) != hipSuccess) { ok = false; return nullptr; }
            c->arena.push_back({ (char *)q, cap });
            c->arena_off = 0;
        }
        char *q = c->arena[c->arena_chunk].base + c->arena_off;
        c->arena_off += bytes;
        if (!src || n == 0) { if (!send_run()) ok = false; return (T *)q; }        // scratch: the run of adjacent uploads ends here
        if (bytes > kStageMax) {
            if (!send_run() || hipMemcpyAsync(q, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream) != hipSuccess) ok = false;
            return (T *)q;
        }
        if (stage_used + bytes > c->stage_cap) {
            // grow: the old buffer may still be read by a copy in flight, so it is kept until the context is destroyed (a handful of doublings at most)
            if (!send_run()) ok = false;
            size_t cap = c->stage_cap ? 2 * c->stage_cap : (size_t)4 << 20;
            while (cap < bytes) cap <<= 1;
            void *h = nullptr;
            if (hipHostMalloc(&h, cap, hipHostMallocDefault) != hipSuccess) { ok = false; return nullptr; }
            c->stage_all.push_back(h); c->stage = (char *)h; c->stage_cap = cap; stage_used = 0;
        }
        if (run_bytes > 0 && q != run_dst + run_bytes) { if (!send_run()) ok = false; }       // not adjacent on the device (a new arena chunk)
        if (run_bytes == 0) { run_dst = q; run_at = stage_used; }
        memcpy(c->stage + stage_used, src, n * sizeof(T));
        stage_used += bytes; run_bytes += bytes;
        return (T *)q;
    }
};
}

#ifdef LMONO_DIAG_SEARCH
extern "C" const char *lmono_version(void) { return "lmono-hip 0.4 (gfx950, diagnostic build: + hash-grid search)"; }
#else
extern "C" const char *lmono_version(void) { return "lmono-hip 0.4 (gfx950)"; }
#endif

extern "C" lmono_ctx *lmono_create(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    lmono_ctx *c = new lmono_ctx();
    c->device = device;
    if (const char *e = getenv("LMONO_ODOM_STREAM_PRIORITY")) c->odom_prio = atoi(e) != 0;
    if (const char *e = getenv("GPU_MAX_HW_QUEUES")) c->many_queues = atoi(e) >= 8;
    if (const char *e = getenv("LMONO_LM_LDS_PLANES")) { const int v = atoi(e); if (lm_planes_valid(v)) c->lm_planes = v; }
    {
        // residency budget of the cluster kernels: every workgroup of a cluster spins on its partners, so all of them must be resident at once.  k_ba_solve
        // takes a whole CU's LDS (one workgroup per CU); half the CUs leaves room for whatever else the card runs (LMONO_CLUSTER_BUDGET overrides: CU masks,
        // CPX partitions report their own multiProcessorCount and need no override)
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) { delete c; return nullptr; }
        c->n_cu = prop.multiProcessorCount;
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_ba_solve<true, false>, kBaT, 0) != hipSuccess || per_cu < 1) per_cu = 1;
        c->cluster_budget = std::max(8, c->n_cu * per_cu / 2);
        c->map_budget = std::max(8, c->n_cu / 2);         // k_map_solve: one workgroup per CU assumed, as measured (more fit, none are counted on)
        if (const char *e = getenv("LMONO_CLUSTER_BUDGET")) { const int v = atoi(e); if (v >= 1) c->cluster_budget = c->map_budget = v; }
    }
    if (hipMalloc((void **)&c->stats_d, 320) != hipSuccess || hipMemset(c->stats_d, 0, 320) != hipSuccess) { delete c; return nullptr; }
    // the selection kernel needs ~62 KB of dynamic LDS
    if (hipFuncSetAttribute((const void *)k_select, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * sel_slice_bytes(kRingCap) + 4 * kSelScratch) != hipSuccess) { delete c; return nullptr; }
    if (hipFuncSetAttribute((const void *)k_voxel<kVoxSmallSlots, kVoxSmallBits, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kVoxLdsSmall) != hipSuccess) { delete c; return nullptr; }
    if (hipFuncSetAttribute((const void *)k_voxel<kVoxBigSlots, kVoxBigBits, false>, hipFuncAttributeMaxDynamicSharedMemorySize, kVoxLdsBig) != hipSuccess) { delete c; return nullptr; }
    if (hipFuncSetAttribute((const void *)k_lm_solve<4>, hipFuncAttributeMaxDynamicSharedMemorySize, lm_rec_lds(4)) != hipSuccess) { delete c; return nullptr; }
#ifdef LMONO_DIAG_SEARCH
    if (hipFuncSetAttribute((const void *)k_grid_build, hipFuncAttributeMaxDynamicSharedMemorySize, kGridLds) != hipSuccess) { delete c; return nullptr; }
#endif
    if (hipFuncSetAttribute((const void *)k_compact_index, hipFuncAttributeMaxDynamicSharedMemorySize, kLiLdsHalf) != hipSuccess) { delete c; return nullptr; }
    if (hipFuncSetAttribute((const void *)k_line_index<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kLiLdsFull) != hipSuccess) { delete c; return nullptr; }
    // the BA-side kernels with large dynamic LDS: per device, so per context (a second context on another GPU needs them too)
    if (hipFuncSetAttribute((const void *)k_marginalize, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(MargLds)) != hipSuccess) { delete c; return nullptr; }
    if (hipFuncSetAttribute((const void *)k_marg_second_new, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Marg2Lds)) != hipSuccess) { delete c; return nullptr; }
#ifdef LMONO_TILE_PROF
    {
        int nb = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k_corr_flat, kCfT, 0);
        std::fprintf(stderr, "[lmono diag] k_corr_flat: %d workgroups of %d threads per CU by the occupancy query, static LDS %zu B\n", nb, kCfT, sizeof(CfLds));
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k_compact_index, kLiT, kLiLdsHalf);
        std::fprintf(stderr, "[lmono diag] k_compact_index: %d workgroups of %d threads per CU by the occupancy query, dynamic LDS %d B\n", nb, kLiT, kLiLdsHalf);
    }
#endif
    return c;
}

extern "C" void lmono_destroy(lmono_ctx *c)
{
    if (!c) return;
#ifdef LMONO_BOUNDS
    {
        // the checked build reports when a context goes (a C++ caller -- estimator_seq -- has no other way to ask)
        unsigned long long o[4] = { 0, 0, 0, 0 };
        (void)hipDeviceSynchronize();
        if (hipMemcpyFromSymbol(o, HIP_SYMBOL(g_ba_oob), sizeof(o)) == hipSuccess)
            fprintf(stderr, "[lmono bounds] k_ba_solve: %llu access(es) outside the batch's allocation (first: ba_solve.hip:%llu, byte offset %lld, block %llu)\n", o[0], o[1], (long long)o[2], o[3]);
    }
#endif
    for (auto &s : c->sets) { for (auto &e : s.e) (void)hipEventDestroy(e); for (auto &e : s.kev) (void)hipEventDestroy(e); }
    if (c->stats_d) (void)hipFree(c->stats_d);
    for (auto &s : c->gstream) if (s) (void)hipStreamDestroy(s);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (void *h : c->stage_all) (void)hipHostFree(h);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    for (auto &ch : c->arena) (void)hipFree(ch.base);
    for (auto &e : c->gev) if (e) (void)hipEventDestroy(e);
    delete c;
}

extern "C" const char *lmono_last_error(const lmono_ctx *c) { return c ? c->err.c_str() : "null context"; }

extern "C" int lmono_set_stream(lmono_ctx *c, void *s)
{
    if (!c) return LMONO_EINVAL;
    c->stream = (hipStream_t)s;
    return LMONO_OK;
}

extern "C" int lmono_use_own_stream(lmono_ctx *c)
{
    if (!c) return LMONO_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->own_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    return LMONO_OK;
}

extern "C" int lmono_set_option(lmono_ctx *c, int key, int value)
{
    if (!c || key < 0 || key >= LMONO_OPT_COUNT) return LMONO_EINVAL;
#ifdef LMONO_DIAG_SEARCH
    const bool grid_search = true;
#else
    const bool grid_search = false;  // the round-1 hash-grid search (0) is compiled into the diagnostic build only
#endif
    const bool ok = key == LMONO_OPT_CORR_TILE ? (value == 3 || (value == 0 && grid_search))
                  : key == LMONO_OPT_DEFER_EVERY ? value >= 0
                  : key == LMONO_OPT_ODOM_STREAMS ? (value >= 1 && value <= 8)
                  : key == LMONO_OPT_BOUNDARY_TOL ? value >= 0
                  : key == LMONO_OPT_BA_CLUSTER ? (value == 0 || value == 1 || value == 2 || value == 4 || value == 8)
                  : key == LMONO_OPT_LEAD_SEED ? (value >= 0 && value <= 1)
                  : value >= -1;                                     // LMONO_OPT_LEAD_FULL
    if (!ok) { c->err = "lmono_set_option: value out of range for this option"; return LMONO_EINVAL; }
    c->opt[key] = value;
    return LMONO_OK;
}

extern "C" int lmono_get_option(lmono_ctx *c, int key, int *value)
{
    if (!c || !value || key < 0 || key >= LMONO_OPT_COUNT) return LMONO_EINVAL;
    *value = c->opt[key];
    return LMONO_OK;
}

extern "C" int lmono_synchronize(lmono_ctx *c)
{
    if (!c) return LMONO_EINVAL;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return LMONO_OK;
}

extern "C" void *lmono_host_alloc(lmono_ctx *c, size_t bytes)
{
    if (!c || bytes == 0 || hipSetDevice(c->device) != hipSuccess) return nullptr;
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { c->err = "lmono_host_alloc: hipHostMalloc failed"; return nullptr; }
    return p;
}
extern "C" void lmono_host_free(lmono_ctx *c, void *p) { if (c && p) (void)hipHostFree(p); }

// hs[s] as the s-th handle of a batched call: a handle of c that no earlier stream names, null or another context's, or hs[u] again (u < s).
// The entry points ask per stream, inside their own loop: which of a stream's faults is reported first, and in which words, stays theirs
enum { kHandleOk = 0, kHandleForeign, kHandleRepeated };
template <typename H> static int batch_handle_fault(const lmono_ctx *c, int s, H *const *hs)
{
    if (!hs[s] || hs[s]->ctx != c) return kHandleForeign;
    for (int u = 0; u < s; u++) if (hs[u] == hs[s]) return kHandleRepeated;
    return kHandleOk;
}

// the two handles of stream s of the batched call `who`, for the entry points that report both kinds alike; nouns: "filters and map builders"
template <typename A, typename B> static bool batch_pair_ok(lmono_ctx *c, const char *who, const char *nouns, int s, A *const *as, B *const *bs)
{
    const int fa = batch_handle_fault(c, s, as), fb = batch_handle_fault(c, s, bs);
    if (fa == kHandleForeign || fb == kHandleForeign) { c->err = std::string(who) + ": bad stream arguments"; return false; }
    if (fa == kHandleRepeated || fb == kHandleRepeated) { c->err = std::string(who) + ": " + nouns + " must be distinct"; return false; }
    return true;
}

// the world cloud of a map builder's last frame, as long as it is still in rgb_map (B: lmono_map_builder, defined in colour_abi.hip)
template <typename B, typename P> static bool builder_last_cloud(lmono_ctx *c, const char *who, const B *b, const P *&pts, int64_t &n)
{
    if (b->last_off + b->last_n > b->map_n) { c->err = std::string(who) + ": the world cloud of a builder's last frame is no longer in rgb_map"; return false; }
    pts = b->map + b->last_off; n = b->last_n;
    return true;
}

// The last result of a handle into the caller's arrays: n items of up to two device arrays (a null destination is skipped), one synchronisation.
// Returns n, or LMONO_ECAPACITY when cap < n
static int64_t read_last(lmono_ctx *c, const char *who, int64_t n, int64_t cap, void *dst0, const void *src0, size_t item0, void *dst1 = nullptr, const void *src1 = nullptr,
                         size_t item1 = 0)
{
    if (cap < n) { c->err = std::string(who) + ": output capacity too small"; return LMONO_ECAPACITY; }
    if (n > 0) {
        if (dst0) HIP_TRY(c, hipMemcpyAsync(dst0, src0, item0 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        if (dst1) HIP_TRY(c, hipMemcpyAsync(dst1, src1, item1 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return n;
}

#include "lidar_abi.hip"
#include "ba_abi.hip"
#include "feat_abi.hip"
#include "mapping_abi.hip"
#include "colour_abi.hip"
#include "voxel_map_abi.hip"
#include "sor_abi.hip"
#include "icp_abi.hip"
#include "normals_abi.hip"
#include "fpfh_abi.hip"
#include "sacia_abi.hip"
#include "track_abi.hip"
#include "keyframe_abi.hip"
#include "pnp_abi.hip"
#include "bow_abi.hip"
#include "posegraph_abi.hip"
#include "excalib_abi.hip"
