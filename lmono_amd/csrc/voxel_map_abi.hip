// voxel_map_abi.hip -- C ABI of the voxel-grid colour map (included by lmono_hip.hip after colour_abi.hip: insert_frames reads a map builder)
#pragma once
#include "voxel_map.hip"
#include "voxel_grow.hpp"

struct lmono_voxel_map {
    lmono_ctx *ctx = nullptr;
    float leaf = 0.0f, inv = 0.0f;
    int64_t max_voxels = 0, n_vox = 0;       // n_vox: voxels with count > 0 (what size / read / cells see)
    int64_t grow_limit = 0, rehashes = 0;    // grow_limit 0: fixed size; rehashes: tables replaced so far (reserve and automatic growth)
    uint64_t slots = 0;
    bool full = false;                       // an insert was refused: every further one is, until clear or reserve
    int form = kVmLdsTable;                  // LMONO_VOXEL_FORM=0 at create (measurement switch): one probe and one set of adds per point instead of the LDS table; a batched call runs in its first map's form
    DevOwner mem;
    VmRec *rec = nullptr;                    // slots records + one 64-B row of counters: one allocation, replaced as one (vm_rebuild)
    unsigned *ctl = nullptr;                 // that row: [0] claimed slots, [1] counter of k_vm_compact
    PtRgb *pts = nullptr;                    // staging of the host-buffer entry
    int64_t pts_cap = 0;
    VmEnt *ent = nullptr;                   // per-call scratch: entries per tile, entry counts
    int64_t ent_cap = 0;                     // in tiles
    unsigned *tile_n = nullptr;
    int64_t tile_cap = 0;
    VmRec *rd_rec = nullptr;                // read / cells: the occupied records
    PtRgb *rd_pts = nullptr;
    int64_t rd_rec_cap = 0, rd_pts_cap = 0;
    // per-call job table + results of a batch led by this map
    VmJob *jobs = nullptr;
    int *results = nullptr;
    int jobs_cap = 0;
    // job table + [2] result ints per map of a rebuild led by this map
    VmGrowJob *grow_jobs = nullptr;
    int *grow_res = nullptr;
    int grow_cap = 0;
    // per-call scratch of a compose into this map: one entry per source voxel, the source table, [4] 64-bit stats + [4] result ints
    VmMoveEnt *mv_ent = nullptr;
    int64_t mv_ent_cap = 0;
    VmMoveSrc *mv_src = nullptr;
    int64_t mv_src_cap = 0;
    unsigned long long *mv_ctl = nullptr;
};

static constexpr int64_t kVmMaxCall = (int64_t)1 << 30;    // points of one insert

extern "C" void lmono_voxel_map_destroy(lmono_voxel_map *m) { delete m; }

static int vm_clear(lmono_ctx *c, lmono_voxel_map *m)
{
    k_vm_clear<<<(unsigned)((m->slots * 8 + kVmT - 1) / kVmT), kVmT, 0, c->stream>>>(m->rec, m->slots);
    if (int rc = check_launch(c, "k_vm_clear")) return rc;
    HIP_TRY(c, hipMemsetAsync(m->ctl, 0, 2 * sizeof(unsigned), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    m->n_vox = 0; m->full = false;
    return LMONO_OK;
}

extern "C" lmono_voxel_map *lmono_voxel_map_create(lmono_ctx *c, float leaf, int64_t max_voxels)
{
    if (!c) return nullptr;
    if (!std::isfinite(leaf) || !(leaf > 0.0f) || max_voxels < 1 || max_voxels > kVmMaxVoxels || !std::isfinite(1.0f / leaf) || !(1.0f / leaf > 0.0f)) {
        c->err = "lmono_voxel_map_create: leaf must be finite and > 0 (with a finite 1 / leaf), max_voxels in 1 .. 2^30";
        return nullptr;
    }
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return nullptr; }
    lmono_voxel_map *m = new lmono_voxel_map();
    m->ctx = c;
    m->leaf = leaf; m->inv = 1.0f / leaf;
    m->max_voxels = max_voxels;
    m->slots = vm_slots(max_voxels);
    if (const char *e = getenv("LMONO_VOXEL_FORM")) { const int v = atoi(e); if (v == kVmPlain || v == kVmLdsTable) m->form = v; }
    const bool ok = m->mem.alloc(m->rec, (size_t)m->slots + 1);
    if (ok) m->ctl = (unsigned *)(m->rec + m->slots);
    if (!ok || vm_clear(c, m) != LMONO_OK) { c->err = "lmono_voxel_map_create: device allocation failed"; lmono_voxel_map_destroy(m); return nullptr; }
    return m;
}

extern "C" int lmono_voxel_map_clear(lmono_ctx *c, lmono_voxel_map *m)
{
    if (!c || !m || m->ctx != c) return LMONO_EINVAL;
    return vm_clear(c, m);
}

// The enqueued part of vm_rebuild: fresh tables cleared, the occupied records of the old ones moved in; res [n][2] as VmGrowJob::res
static int vm_rebuild_run(lmono_ctx *c, lmono_voxel_map *lead, const std::vector<VmGrowJob> &jobs, std::vector<int> &res)
{
    const int n = (int)jobs.size();
    uint64_t clear_rows = 0, src_slots = 0;
    for (const VmGrowJob &j : jobs) { clear_rows = std::max<uint64_t>(clear_rows, j.dst_slots + 1); src_slots = std::max<uint64_t>(src_slots, j.src_slots); }
    HIP_TRY(c, hipMemcpyAsync(lead->grow_jobs, jobs.data(), sizeof(VmGrowJob) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(lead->grow_res, 0, sizeof(int) * 2 * (size_t)n, c->stream));
    k_vm_clear_jobs<<<dim3((unsigned)((clear_rows * 8 + kVmT - 1) / kVmT), (unsigned)n), kVmT, 0, c->stream>>>(lead->grow_jobs);
    if (int rc = check_launch(c, "k_vm_clear_jobs")) return rc;
    if (src_slots) {                                            // only empty maps: nothing to move, no launch
        k_vm_rehash<<<dim3((unsigned)((src_slots + kVmTile - 1) / kVmTile), (unsigned)n), kVmT, 0, c->stream>>>(lead->grow_jobs);
        if (int rc = check_launch(c, "k_vm_rehash")) return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(res.data(), lead->grow_res, sizeof(int) * res.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return LMONO_OK;
}

// Rebuild n distinct maps, map s for max_voxels[s] >= its size: all fresh tables are allocated first, then one clear launch and one rehash launch
// for all maps (ghost claims of refused calls are dropped), and the old tables go only when every new one has been checked.  On any failure no map
// has changed.  Ends synchronised, like every entry point here, so nothing in flight reads a released table.
static int vm_rebuild(lmono_ctx *c, const char *who, int n, lmono_voxel_map *const *maps, const int64_t *max_voxels)
{
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return LMONO_ENODEV; }
    lmono_voxel_map *lead = maps[0];
    std::vector<VmRec *> fresh((size_t)n, nullptr);
    auto drop = [&] { for (int s = 0; s < n; s++) maps[s]->mem.release(fresh[(size_t)s]); };
    bool ok = true;
    for (int s = 0; s < n && ok; s++) ok = maps[s]->mem.alloc(fresh[(size_t)s], (size_t)vm_slots(max_voxels[s]) + 1);
    ok = ok && job_table(lead->mem, lead->grow_jobs, lead->grow_res, lead->grow_cap, n, 2);
    if (!ok) { drop(); c->err = std::string(who) + ": allocation of the new tables failed; no map was changed"; return LMONO_ENOMEM; }
    std::vector<VmGrowJob> jobs((size_t)n);
    for (int s = 0; s < n; s++) {
        VmGrowJob &j = jobs[(size_t)s];
        j.src = maps[s]->rec; j.src_slots = maps[s]->n_vox ? maps[s]->slots : 0;
        j.dst = fresh[(size_t)s]; j.dst_slots = vm_slots(max_voxels[s]);
        j.res = lead->grow_res + 2 * s;
    }
    std::vector<int> res((size_t)n * 2);
    if (int rc = vm_rebuild_run(c, lead, jobs, res)) { (void)hipStreamSynchronize(c->stream); drop(); return rc; }
    for (int s = 0; s < n; s++)
        if (res[2 * (size_t)s] != 0 || (int64_t)(unsigned)res[2 * (size_t)s + 1] != maps[s]->n_vox) {
            drop();
            c->err = std::string(who) + ": table inconsistent (the records moved into the new table do not match the map's size); no map was changed";
            return LMONO_ENODEV;
        }
    for (int s = 0; s < n; s++) {
        lmono_voxel_map *m = maps[s];
        m->mem.release(m->rec);
        m->rec = fresh[(size_t)s];
        m->max_voxels = max_voxels[s]; m->slots = vm_slots(max_voxels[s]);
        m->ctl = (unsigned *)(m->rec + m->slots);
        m->full = false; m->rehashes++;
    }
    return LMONO_OK;
}

extern "C" int lmono_voxel_map_reserve(lmono_ctx *c, int n, lmono_voxel_map *const *maps, const int64_t *max_voxels)
{
    if (!c || n <= 0 || !maps || !max_voxels) return LMONO_EINVAL;
    for (int s = 0; s < n; s++) {
        const int fault = batch_handle_fault(c, s, maps);
        if (fault == kHandleForeign) { c->err = "lmono_voxel_map_reserve: bad map handle"; return LMONO_EINVAL; }
        if (fault == kHandleRepeated) { c->err = "lmono_voxel_map_reserve: the maps must be distinct"; return LMONO_EINVAL; }
        if (max_voxels[s] < 1 || max_voxels[s] < maps[s]->n_vox || max_voxels[s] > kVmMaxVoxels) {
            c->err = "lmono_voxel_map_reserve: max_voxels must be in max(size, 1) .. 2^30";
            return LMONO_EINVAL;
        }
    }
    return vm_rebuild(c, "lmono_voxel_map_reserve", n, maps, max_voxels);
}

extern "C" int lmono_voxel_map_set_growth(lmono_ctx *c, lmono_voxel_map *m, int64_t limit_voxels)
{
    if (!c || !m || m->ctx != c) return LMONO_EINVAL;
    if (limit_voxels != 0 && (limit_voxels < m->max_voxels || limit_voxels > kVmMaxVoxels)) {
        c->err = "lmono_voxel_map_set_growth: the limit must be 0 (fixed size) or in max_voxels .. 2^30";
        return LMONO_EINVAL;
    }
    m->grow_limit = limit_voxels;
    return LMONO_OK;
}

extern "C" int lmono_voxel_map_capacity(lmono_ctx *c, lmono_voxel_map *m, int64_t out[4])
{
    if (!c || !m || m->ctx != c || !out) return LMONO_EINVAL;
    out[0] = m->max_voxels; out[1] = (int64_t)m->slots; out[2] = m->grow_limit; out[3] = m->rehashes;
    return LMONO_OK;
}

// one insert for n maps: pts_d[s] device clouds of ns[s] points.  Two launches in all, unless a refused stream's map may grow: then those maps are
// rebuilt one step larger (vm_rebuild) and the two launches repeated for those streams only, until each fits or stands at its limit.  Ends synchronised.
static int vm_insert_batch(lmono_ctx *c, const char *who, int n, lmono_voxel_map *const *maps, const PtRgb *const *pts_d, const int64_t *ns, int64_t *stats)
{
    int64_t max_n = 0;
    for (int s = 0; s < n; s++) {
        lmono_voxel_map *m = maps[s];
        if (m->full) { c->err = std::string(who) + ": the map is full (an insert needed more than max_voxels voxels; clear it or create it larger)"; return LMONO_ECAPACITY; }
        max_n = std::max(max_n, ns[s]);
    }
    if (stats)
        for (int s = 0; s < n; s++) { stats[4 * s] = stats[4 * s + 1] = stats[4 * s + 2] = 0; stats[4 * s + 3] = maps[s]->n_vox; }
    if (max_n == 0) return LMONO_OK;                           // nothing to do: no launch
    lmono_voxel_map *lead = maps[0];
    if (!job_table(lead->mem, lead->jobs, lead->results, lead->jobs_cap, n, 4)) { c->err = std::string(who) + ": job table allocation failed"; return LMONO_ENOMEM; }
    std::vector<int> act((size_t)n), grow;                      // streams of this round (job k is stream act[k]); refused streams whose maps may grow
    for (int s = 0; s < n; s++) act[(size_t)s] = s;
    std::vector<VmJob> jobs;
    std::vector<int> res;
    int rc = LMONO_OK;
    for (;;) {
        const int na = (int)act.size();
        jobs.resize((size_t)na);
        max_n = 0;
        for (int k = 0; k < na; k++) {
            const int s = act[(size_t)k];
            lmono_voxel_map *m = maps[s];
            const int64_t tiles = (ns[s] + kVmTile - 1) / kVmTile;
            // every insert ends synchronised, so nothing in flight reads an outgrown scratch (grow_replace)
            if (!m->mem.grow_replace(m->ent, m->ent_cap, (size_t)tiles, /*floor=*/64, /*per=*/kVmTile) || !m->mem.grow_replace(m->tile_n, m->tile_cap, (size_t)tiles, /*floor=*/64)) {
                c->err = std::string(who) + ": scratch allocation failed"; return LMONO_ENOMEM;
            }
            VmJob &j = jobs[(size_t)k];
            j.pts = pts_d[s]; j.n = ns[s];
            j.rec = m->rec; j.occ = m->ctl; j.mask = (unsigned)(m->slots - 1); j.max_voxels = (unsigned)m->max_voxels; j.inv = m->inv;
            j.ent = m->ent; j.tile_n = m->tile_n; j.res = lead->results + 4 * k;
            max_n = std::max(max_n, ns[s]);
        }
        HIP_TRY(c, hipMemcpyAsync(lead->jobs, jobs.data(), sizeof(VmJob) * (size_t)na, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(lead->results, 0, sizeof(int) * 4 * (size_t)na, c->stream));
        const dim3 grid((unsigned)((max_n + kVmTile - 1) / kVmTile), (unsigned)na);
        if (lead->form == kVmPlain) k_vm_find<kVmPlain><<<grid, kVmT, 0, c->stream>>>(lead->jobs);
        else k_vm_find<kVmLdsTable><<<grid, kVmT, 0, c->stream>>>(lead->jobs);
        if (int e = check_launch(c, "k_vm_find")) return e;
        k_vm_accum<<<grid, kVmT, 0, c->stream>>>(lead->jobs);
        if (int e = check_launch(c, "k_vm_accum")) return e;
        res.resize((size_t)na * 4);
        HIP_TRY(c, hipMemcpyAsync(res.data(), lead->results, sizeof(int) * res.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        grow.clear();
        for (int k = 0; k < na; k++) {
            const int s = act[(size_t)k];
            lmono_voxel_map *m = maps[s];
            if (ns[s] == 0) continue;
            const int *r = res.data() + 4 * (size_t)k;
            if (stats) stats[4 * s + 1] = r[1];
            if (r[0]) {                                         // nothing of this call is in the map; keys it claimed stay with count 0, unseen
                m->full = true;                                 // ... and so it stays if the map cannot grow, or the growth fails
                if (m->grow_limit > m->max_voxels) { grow.push_back(s); continue; }
                c->err = std::string(who) + ": the points need more than max_voxels voxels; nothing was inserted and the map is full until cleared or rebuilt (lmono_voxel_map_reserve)";
                rc = LMONO_ECAPACITY;
                continue;
            }
            if (stats) { stats[4 * s] = r[2]; stats[4 * s + 2] = (int64_t)(unsigned)r[3] - m->n_vox; stats[4 * s + 3] = (int64_t)(unsigned)r[3]; }
            m->n_vox = (int64_t)(unsigned)r[3];
        }
        if (grow.empty()) return rc;
        // a refused call inserted nothing, so the same streams go in again once their maps are one step larger and rid of the ghost claims
        std::vector<lmono_voxel_map *> gm;
        std::vector<int64_t> gv;
        for (int s : grow) { gm.push_back(maps[s]); gv.push_back(vm_grow_step(maps[s]->max_voxels, maps[s]->grow_limit)); }
        if (int e = vm_rebuild(c, who, (int)gm.size(), gm.data(), gv.data())) return e;      // those maps stay full; a later reserve repairs them
        act = grow;
    }
}

extern "C" int lmono_voxel_map_insert_d(lmono_ctx *c, lmono_voxel_map *m, const lmono_point_rgb *pts_d, int64_t n, int64_t *stats)
{
    if (!c || !m || m->ctx != c || n < 0 || (n > 0 && !pts_d)) return LMONO_EINVAL;
    if (n > kVmMaxCall) { c->err = "lmono_voxel_map_insert: more than 2^30 points in one call"; return LMONO_EINVAL; }
    const PtRgb *p = (const PtRgb *)pts_d;
    return vm_insert_batch(c, "lmono_voxel_map_insert", 1, &m, &p, &n, stats);
}

extern "C" int lmono_voxel_map_insert(lmono_ctx *c, lmono_voxel_map *m, const lmono_point_rgb *pts_h, int64_t n, int64_t *stats)
{
    if (!c || !m || m->ctx != c || n < 0 || (n > 0 && !pts_h)) return LMONO_EINVAL;
    if (n > kVmMaxCall) { c->err = "lmono_voxel_map_insert: more than 2^30 points in one call"; return LMONO_EINVAL; }
    if (n > 0 && !m->full) {
        if (!m->mem.grow_replace(m->pts, m->pts_cap, (size_t)n, /*floor=*/1 << 16)) { c->err = "lmono_voxel_map_insert: staging allocation failed"; return LMONO_ENOMEM; }
        HIP_TRY(c, hipMemcpyAsync(m->pts, pts_h, sizeof(PtRgb) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    const PtRgb *p = m->pts;
    const int rc = vm_insert_batch(c, "lmono_voxel_map_insert", 1, &m, &p, &n, stats);
    if (rc != LMONO_OK) (void)hipStreamSynchronize(c->stream);      // an early return must not leave the copy from the caller's buffer in flight
    return rc;
}

extern "C" int lmono_voxel_map_insert_frames(lmono_ctx *c, int n, lmono_voxel_map *const *maps, lmono_map_builder *const *mbs, int64_t *stats)
{
    if (!c || n <= 0 || !maps || !mbs) return LMONO_EINVAL;
    std::vector<const PtRgb *> pts((size_t)n);
    std::vector<int64_t> ns((size_t)n);
    for (int s = 0; s < n; s++) {
        if (!batch_pair_ok(c, "lmono_voxel_map_insert_frames", "maps and map builders", s, maps, mbs)) return LMONO_EINVAL;
        if (!builder_last_cloud(c, "lmono_voxel_map_insert_frames", mbs[s], pts[(size_t)s], ns[(size_t)s])) return LMONO_EINVAL;
    }
    return vm_insert_batch(c, "lmono_voxel_map_insert_frames", n, maps, pts.data(), ns.data(), stats);
}

extern "C" int64_t lmono_voxel_map_size(lmono_ctx *c, lmono_voxel_map *m)
{
    if (!c || !m || m->ctx != c) return LMONO_EINVAL;
    return m->n_vox;
}

// the occupied records in ascending key order: compacted on the device, ordered on the host (the read ends in host memory and is no hot path)
static int vm_collect(lmono_ctx *c, lmono_voxel_map *m, std::vector<VmRec> &recs)
{
    recs.clear();
    if (m->n_vox == 0) return LMONO_OK;
    if (!m->mem.grow_replace(m->rd_rec, m->rd_rec_cap, (size_t)m->n_vox, /*floor=*/1024)) { c->err = "lmono_voxel_map: read buffer allocation failed"; return LMONO_ENOMEM; }
    HIP_TRY(c, hipMemsetAsync(m->ctl + 1, 0, sizeof(unsigned), c->stream));
    k_vm_compact<<<(unsigned)((m->slots + kVmT - 1) / kVmT), kVmT, 0, c->stream>>>(m->rec, m->slots, m->rd_rec, (unsigned)m->n_vox, m->ctl + 1);
    if (int rc = check_launch(c, "k_vm_compact")) return rc;
    unsigned found = 0;
    HIP_TRY(c, hipMemcpyAsync(&found, m->ctl + 1, sizeof found, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((int64_t)found != m->n_vox) { c->err = "lmono_voxel_map: the table's occupied records do not match its size"; return LMONO_ENODEV; }
    recs.resize((size_t)found);
    HIP_TRY(c, hipMemcpy(recs.data(), m->rd_rec, sizeof(VmRec) * recs.size(), hipMemcpyDeviceToHost));
    std::sort(recs.begin(), recs.end(), [](const VmRec &a, const VmRec &b) { return a.key < b.key; });
    return LMONO_OK;
}

// a non-empty map as another stage's input cloud: its output points into out_d[n_vox] in any order, their number into *found_d (the caller
// compares it with n_vox once its own call has synchronised).  One launch, no wait
static int vm_enqueue_points(lmono_ctx *c, const lmono_voxel_map *m, PtRgb *out_d, unsigned *found_d)
{
    HIP_TRY(c, hipMemsetAsync(found_d, 0, sizeof(unsigned), c->stream));
    k_vm_points_unordered<<<(unsigned)((m->slots + kVmT - 1) / kVmT), kVmT, 0, c->stream>>>(m->rec, m->slots, m->leaf, out_d, (unsigned)m->n_vox, found_d);
    return check_launch(c, "k_vm_points_unordered");
}

extern "C" int64_t lmono_voxel_map_cells(lmono_ctx *c, lmono_voxel_map *m, uint64_t *keys_h, uint32_t *counts_h, uint64_t *sums_h, int64_t cap)
{
    if (!c || !m || m->ctx != c) return LMONO_EINVAL;
    if (!keys_h && !counts_h && !sums_h) return m->n_vox;
    if (cap < m->n_vox) { c->err = "lmono_voxel_map_cells: output capacity too small"; return LMONO_ECAPACITY; }
    std::vector<VmRec> recs;
    if (int rc = vm_collect(c, m, recs)) return rc;
    for (size_t i = 0; i < recs.size(); i++) {
        if (keys_h) keys_h[i] = recs[i].key;
        if (counts_h) counts_h[i] = (uint32_t)recs[i].w[0];
        if (sums_h) for (int w = 0; w < 6; w++) sums_h[6 * i + w] = recs[i].w[1 + w];
    }
    return m->n_vox;
}

extern "C" int64_t lmono_voxel_map_read(lmono_ctx *c, lmono_voxel_map *m, lmono_point_rgb *out_h, int64_t cap)
{
    if (!c || !m || m->ctx != c) return LMONO_EINVAL;
    if (!out_h) return m->n_vox;
    if (cap < m->n_vox) { c->err = "lmono_voxel_map_read: output capacity too small"; return LMONO_ECAPACITY; }
    std::vector<VmRec> recs;
    if (int rc = vm_collect(c, m, recs)) return rc;
    if (recs.empty()) return 0;
    if (!m->mem.grow_replace(m->rd_pts, m->rd_pts_cap, recs.size(), /*floor=*/1024)) { c->err = "lmono_voxel_map_read: output buffer allocation failed"; return LMONO_ENOMEM; }
    HIP_TRY(c, hipMemcpyAsync(m->rd_rec, recs.data(), sizeof(VmRec) * recs.size(), hipMemcpyHostToDevice, c->stream));
    k_vm_finish<<<(unsigned)((recs.size() + kVmT - 1) / kVmT), kVmT, 0, c->stream>>>(m->rd_rec, (unsigned)recs.size(), m->leaf, m->rd_pts);
    if (int rc = check_launch(c, "k_vm_finish")) return rc;
    HIP_TRY(c, hipMemcpyAsync(out_h, m->rd_pts, sizeof(PtRgb) * recs.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return m->n_vox;
}

// fold n_src maps, each moved by its transform, into dst: one k_vm_compact per non-empty source into that source's read buffer,
// then two launches for all sources.  Ends synchronised.
extern "C" int lmono_voxel_map_compose(lmono_ctx *c, lmono_voxel_map *dst, int n_src, lmono_voxel_map *const *srcs, const double *transforms, int64_t *stats)
{
    const char *who = "lmono_voxel_map_compose";
    if (!c || !dst || dst->ctx != c || n_src < 0 || (n_src > 0 && (!srcs || !transforms))) return LMONO_EINVAL;
    if (n_src > 65535) { c->err = std::string(who) + ": more than 65535 sources in one call"; return LMONO_EINVAL; }
    int64_t total = 0;
    for (int s = 0; s < n_src; s++) {
        const int fault = batch_handle_fault(c, s, srcs);
        if (fault == kHandleForeign) { c->err = std::string(who) + ": bad source handle"; return LMONO_EINVAL; }
        if (fault == kHandleRepeated || srcs[s] == dst) { c->err = std::string(who) + ": the sources must be distinct, and none of them the destination"; return LMONO_EINVAL; }
        total += srcs[s]->n_vox;
    }
    for (int64_t k = 0; k < 12 * (int64_t)n_src; k++)
        if (!std::isfinite(transforms[k])) { c->err = std::string(who) + ": non-finite transform entry"; return LMONO_EINVAL; }
    if (total > kVmMaxCall) { c->err = std::string(who) + ": more than 2^30 source voxels in one call"; return LMONO_EINVAL; }
    if (dst->full) { c->err = std::string(who) + ": the map is full (an insert needed more than max_voxels voxels; clear it or create it larger)"; return LMONO_ECAPACITY; }
    if (stats) { for (int k = 0; k < 5; k++) stats[k] = 0; stats[5] = dst->n_vox; }
    if (total == 0) return LMONO_OK;                            // nothing to do: no launch
    if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return LMONO_ENODEV; }
    // every compose ends synchronised, so nothing in flight reads an outgrown scratch (grow_replace)
    if ((!dst->mv_ctl && !dst->mem.alloc(dst->mv_ctl, 6)) || !dst->mem.grow_replace(dst->mv_ent, dst->mv_ent_cap, (size_t)total, /*floor=*/1024) ||
        !dst->mem.grow_replace(dst->mv_src, dst->mv_src_cap, (size_t)n_src, /*floor=*/1)) {
        c->err = std::string(who) + ": scratch allocation failed"; return LMONO_ENOMEM;
    }
    std::vector<VmMoveSrc> tab((size_t)n_src);
    int64_t off = 0, max_n = 0;
    for (int s = 0; s < n_src; s++) {
        lmono_voxel_map *m = srcs[s];
        VmMoveSrc &t = tab[(size_t)s];
        t.rec = nullptr; t.n = (unsigned)m->n_vox; t.leaf = m->leaf; t.ent_off = off;
        for (int k = 0; k < 12; k++) t.T[k] = transforms[12 * (size_t)s + k];
        if (m->n_vox == 0) continue;
        if (!m->mem.grow_replace(m->rd_rec, m->rd_rec_cap, (size_t)m->n_vox, /*floor=*/1024)) { c->err = std::string(who) + ": read buffer allocation failed"; return LMONO_ENOMEM; }
        HIP_TRY(c, hipMemsetAsync(m->ctl + 1, 0, sizeof(unsigned), c->stream));
        k_vm_compact<<<(unsigned)((m->slots + kVmT - 1) / kVmT), kVmT, 0, c->stream>>>(m->rec, m->slots, m->rd_rec, (unsigned)m->n_vox, m->ctl + 1);
        if (int rc = check_launch(c, "k_vm_compact")) return rc;
        t.rec = m->rd_rec;
        off += m->n_vox; max_n = std::max(max_n, m->n_vox);
    }
    HIP_TRY(c, hipMemcpyAsync(dst->mv_src, tab.data(), sizeof(VmMoveSrc) * tab.size(), hipMemcpyHostToDevice, c->stream));
    const dim3 grid((unsigned)((max_n + kVmTile - 1) / kVmTile), (unsigned)n_src);
    unsigned long long ctl[6];
    int res[4];
    for (;;) {                                                  // once, unless dst is refused and may grow: then one step larger and again
        VmJob j{};
        j.rec = dst->rec; j.occ = dst->ctl; j.mask = (unsigned)(dst->slots - 1); j.max_voxels = (unsigned)dst->max_voxels; j.inv = dst->inv;
        j.res = (int *)(dst->mv_ctl + 4);
        HIP_TRY(c, hipMemsetAsync(dst->mv_ctl, 0, 6 * sizeof(unsigned long long), c->stream));
        k_vm_move_find<<<grid, kVmT, 0, c->stream>>>(j, dst->mv_src, dst->mv_ent, dst->mv_ctl);
        if (int rc = check_launch(c, "k_vm_move_find")) return rc;
        k_vm_move_accum<<<grid, kVmT, 0, c->stream>>>(j, dst->mv_src, dst->mv_ent);
        if (int rc = check_launch(c, "k_vm_move_accum")) return rc;
        HIP_TRY(c, hipMemcpyAsync(ctl, dst->mv_ctl, sizeof ctl, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::memcpy(res, ctl + 4, sizeof res);
        if (!res[0]) break;
        dst->full = true;                                       // nothing of this call is in the map; keys it claimed stay with count 0, unseen
        if (dst->grow_limit <= dst->max_voxels) {
            c->err = std::string(who) + ": the sources need more than max_voxels voxels; nothing was composed and the map is full until cleared or rebuilt (lmono_voxel_map_reserve)";
            return LMONO_ECAPACITY;
        }
        const int64_t next = vm_grow_step(dst->max_voxels, dst->grow_limit);
        if (int rc = vm_rebuild(c, who, 1, &dst, &next)) return rc;      // dst stays full; a later reserve repairs it
    }
    if (stats) { for (int k = 0; k < 4; k++) stats[k] = (int64_t)ctl[k]; stats[4] = (int64_t)(unsigned)res[3] - dst->n_vox; stats[5] = (int64_t)(unsigned)res[3]; }
    dst->n_vox = (int64_t)(unsigned)res[3];
    return LMONO_OK;
}

/* tile size of k_vm_find, for tests that place point counts around it */
extern "C" int lmono_voxel_map_tile(void) { return kVmTile; }
