// voxel_map.hip -- the voxel-grid global colour map on gfx950: the filter MapBuilder::processMapping left commented out
// (mono_lidar_mapping/src/map_builder/Map_Builder.cc:82-98), as a device-resident hash table of exact integer sums.
//
// The table is open addressing over a power of two of 64-B records (VmRec: key, count, six sums), linear probing from vm_mix(key).
// One insert is two launches for all streams (blockIdx.y = stream), because whether a frame fits is known only when every key has been looked up:
//   k_vm_find<1>      a workgroup sums its tile of kVmTile points in an LDS table (64-bit LDS compare-and-swap on the key, 32-bit LDS adds), then
//                      every distinct key of the tile finds its slot in HBM or claims an empty one, and the tile's sums leave as one 32-B entry
//                      per distinct key (slot, count, six sums).
//   k_vm_find<0>      the plain form (the correctness baseline and the measured alternative, LMONO_VOXEL_FORM=0): one probe and one entry per point.
//                      (A segmented wave reduction over runs of equal keys in front of the LDS table was measured too and changed nothing: profiles/r11.)
//   k_vm_accum        does nothing when the stream's failure word is set; otherwise adds every entry to its record: eight lanes per entry, lane w
//                      one 64-bit no-return atomic add on word w of the 64-B record, so a wave instruction is eight whole 64-B rows.
// A claim is a 64-bit compare-and-swap on an empty key; a workgroup then takes one block of tickets from the map's occupancy counter for the slots it
// claimed, and a ticket >= max_voxels sets the failure word.  (Ticket first, as one would write it, refuses a frame that fits: two workgroups that race
// for the same new key both hold a ticket for a moment.  One ticket per claim is exact too but puts every claim of a map on one word: 7.6 ms instead of
// 3.3 for 64 first frames, profiles/r11.)  Once the failure word is set, or the counter has reached max_voxels, no further slot is claimed, and every
// probe loop ends after `slots` steps: no wave waits on the table, whatever is in it.
// Sums are integers, so the content is the same bytes for every insertion order, split, batch and launch geometry.
// A live table changes size by k_vm_clear_jobs / k_vm_rehash below: fresh tables for any number of maps, the occupied records moved into them.
// Whole maps are folded into another one, each under a rigid transform and every voxel with its weight, by k_vm_move_find / k_vm_move_accum below
// (DESIGN.md 6c-4): the same claim, ticket and refusal rules, 64-bit entries.
#pragma once
#include "common.hpp"
#include "colour.hip"
#include "voxel_map.hpp"

namespace lmono {

constexpr int kVmT = 256;                 // threads of every kernel here
constexpr int kVmTile = 512;              // points per workgroup of k_vm_find
constexpr int kVmLds = 2 * kVmTile;      // slots of the workgroup's LDS table (load <= 1/2)
constexpr unsigned kVmNoSlot = 0xffffffffu;
constexpr int kVmRehashU = 4;              // records a group of eight lanes of k_vm_rehash has in flight
static_assert(kVmTile * 8 / kVmT % kVmRehashU == 0, "k_vm_rehash unroll");

struct VmEnt { unsigned slot, w[7]; };    // sums of one distinct key of a tile (or of one point), on their way to record `slot`

struct VmJob {
    const PtRgb *pts;
    long long n;
    VmRec *rec;
    unsigned *occ;                         // claimed slots of the map
    unsigned mask, max_voxels;             // slots - 1
    float inv;
    VmEnt *ent;                           // [tiles][kVmTile]
    unsigned *tile_n;                      // [tiles] entries of each tile
    int *res;                              // [0] failure word, [1] points rejected, [2] points accepted, [3] occupancy after the call
};

static_assert(sizeof(VmRec) == 64 && sizeof(VmEnt) == 32 && sizeof(VmPoint) == sizeof(PtRgb), "voxel map layouts");

// slot of `key`, claimed if new (counted in the workgroup's *claims); kVmNoSlot with the failure word set when the map is full or the probe ran out
__device__ inline unsigned vm_find_or_claim(const VmJob &j, uint64_t key, unsigned *claims)
{
    unsigned h = (unsigned)vm_mix(key) & j.mask;
    for (unsigned probe = 0; probe <= j.mask; probe++, h = (h + 1) & j.mask) {
        unsigned long long *kp = (unsigned long long *)&j.rec[h].key;
        unsigned long long k = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kVmEmpty) {
            if (__hip_atomic_load(j.res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return kVmNoSlot;   // the call is refused already: claim nothing more
            if (__hip_atomic_load(j.occ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= j.max_voxels) {
                // the counter holds the tickets taken so far, never more than the slots claimed.  If this slot is empty NOW, the key is not in the
                // table (its probe path up to here is full of other keys, and slots never change back) while max_voxels other keys are: it cannot fit
                k = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (k == kVmEmpty) { atomicExch(j.res, 1); return kVmNoSlot; }
            } else {
                k = atomicCAS(kp, (unsigned long long)kVmEmpty, (unsigned long long)key);
                if (k == kVmEmpty) { atomicAdd(claims, 1u); return h; }
            }
        }
        if (k == key) return h;
        if ((probe & 31u) == 31u && __hip_atomic_load(j.res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return kVmNoSlot;
    }
    atomicExch(j.res, 1);
    return kVmNoSlot;
}

// the workgroup's LDS table: add the sums v of `key`
__device__ inline void vm_lds_add(unsigned long long *lkey, unsigned (*lacc)[kVmLds], uint64_t key, const unsigned v[7])
{
    unsigned h = (unsigned)(vm_mix(key) >> 40) & (kVmLds - 1);
    for (int probe = 0; probe < kVmLds; probe++, h = (h + 1) & (kVmLds - 1)) {    // at most kVmTile keys in 2 * kVmTile slots: always ends early
        const unsigned long long k = atomicCAS(&lkey[h], (unsigned long long)kVmEmpty, (unsigned long long)key);
        if (k == kVmEmpty || k == key) {
            for (int w = 0; w < 7; w++) atomicAdd(&lacc[w][h], v[w]);                 // <= 512 * 65535 per word
            return;
        }
    }
}

enum { kVmPlain = 0, kVmLdsTable = 1 };

template <int kForm> __global__ __launch_bounds__(kVmT) void k_vm_find(const VmJob *jobs)
{
    constexpr bool kAggregate = kForm != kVmPlain;
    const VmJob &j = jobs[blockIdx.y];
    const long long base = (long long)blockIdx.x * kVmTile;
    if (base >= j.n) return;
    __shared__ unsigned long long lkey[kAggregate ? kVmLds : 1];
    __shared__ unsigned lacc[kAggregate ? 7 : 1][kAggregate ? kVmLds : 1];
    __shared__ unsigned l_n, l_rej, l_claims;
    const int tid = threadIdx.x;
    if constexpr (kAggregate)
        for (int s = tid; s < kVmLds; s += kVmT) {
            lkey[s] = kVmEmpty;
            for (int w = 0; w < 7; w++) lacc[w][s] = 0;
        }
    if (tid == 0) { l_n = 0; l_rej = 0; l_claims = 0; }
    __syncthreads();
    for (int r = 0; r < kVmTile / kVmT; r++) {
        const long long p = base + r * kVmT + tid;
        const bool in = p < j.n;
        PtRgb pt = { 0.0f, 0.0f, 0.0f, 0u };
        if (in) pt = j.pts[p];
        uint64_t key = kVmEmpty;
        int q[3] = { 0, 0, 0 };
        const bool ok = in && vm_cell(pt.x, pt.y, pt.z, j.inv, key, q);
        if (in && !ok) atomicAdd(&l_rej, 1u);
        unsigned add[7] = { 1u, (unsigned)q[0], (unsigned)q[1], (unsigned)q[2], pt.bgra >> 16 & 255u, pt.bgra >> 8 & 255u, pt.bgra & 255u };
        if constexpr (kAggregate) {
            if (ok) vm_lds_add(lkey, lacc, key, add);
        } else if (in) {
            VmEnt e;
            e.slot = ok ? vm_find_or_claim(j, key, &l_claims) : kVmNoSlot;
            for (int w = 0; w < 7; w++) e.w[w] = add[w];
            j.ent[p] = e;
        }
    }
    __syncthreads();
    if constexpr (kAggregate)
        for (int s = tid; s < kVmLds; s += kVmT) {
            const unsigned long long key = lkey[s];
            if (key == kVmEmpty) continue;
            VmEnt e;
            e.slot = vm_find_or_claim(j, key, &l_claims);
            for (int w = 0; w < 7; w++) e.w[w] = lacc[w][s];
            j.ent[base + atomicAdd(&l_n, 1u)] = e;                                       // <= kVmTile distinct keys: inside the tile's part of ent
        }
    __syncthreads();
    if (tid == 0) {
        const long long left = j.n - base;
        j.tile_n[blockIdx.x] = kAggregate ? l_n : (unsigned)(left < kVmTile ? left : kVmTile);
        // one block of tickets for the slots this workgroup claimed: a ticket >= max_voxels refuses the call
        if (l_claims && atomicAdd(j.occ, l_claims) + l_claims > j.max_voxels) atomicExch(j.res, 1);
        if (l_rej) atomicAdd(j.res + 1, (int)l_rej);
        const int in_tile = (int)(left < kVmTile ? left : kVmTile) - (int)l_rej;
        if (in_tile) atomicAdd(j.res + 2, in_tile);
    }
}

__global__ __launch_bounds__(kVmT) void k_vm_accum(const VmJob *jobs)
{
    const VmJob &j = jobs[blockIdx.y];
    const long long base = (long long)blockIdx.x * kVmTile;
    if (base >= j.n) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) j.res[3] = (int)*j.occ;
    if (j.res[0] != 0) return;                 // the frame does not fit: nothing of it enters the map
    const unsigned n = j.tile_n[blockIdx.x];
    const int w = threadIdx.x & 7;
    for (unsigned e = threadIdx.x >> 3; e < n; e += kVmT / 8) {
        const VmEnt *en = j.ent + base + e;
        const unsigned slot = en->slot;
        if (slot == kVmNoSlot || w == 0) continue;      // word 0 of a record is its key
        const unsigned v = en->w[w - 1];
        if (v) atomicAdd((unsigned long long *)&j.rec[slot].w[w - 1], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(kVmT) void k_vm_clear(VmRec *rec, unsigned long long slots)
{
    // eight lanes per record: coalesced 64-B rows
    const unsigned long long i = (unsigned long long)blockIdx.x * kVmT + threadIdx.x;
    if (i >= slots * 8) return;
    ((uint64_t *)rec)[i] = (i & 7) == 0 ? kVmEmpty : 0ull;
}

// ---- a live table changes size: fresh tables cleared, then the old tables' records moved into them; blockIdx.y = map ----
// A table is slots records and one more 64-B row behind them that holds the map's counters (lmono_voxel_map::ctl), so a table and its occupancy
// counter are replaced together and the old pair stands untouched until the new one has been checked.
struct VmGrowJob {
    const VmRec *src;                      // the old table; src_slots == 0: nothing to move (an empty map)
    unsigned long long src_slots;
    VmRec *dst;                            // the fresh table: dst_slots records + the counter row
    unsigned long long dst_slots;
    int *res;                              // [0] failure word, [1] records moved
};

__global__ __launch_bounds__(kVmT) void k_vm_clear_jobs(const VmGrowJob *jobs)
{
    const VmGrowJob &j = jobs[blockIdx.y];
    const unsigned long long i = (unsigned long long)blockIdx.x * kVmT + threadIdx.x;
    if (i >= (j.dst_slots + 1) * 8) return;
    ((uint64_t *)j.dst)[i] = (i & 7) == 0 && i < j.dst_slots * 8 ? kVmEmpty : 0ull;     // the counter row is all zero
}

// Eight lanes per record, lane w word w, on both sides: the old table is read once in whole 64-B rows, a record with a key and count > 0 is
// moved (count 0: the ghost claim of a refused call, dropped).  Lane 0 of the group claims the slot -- keys of one table are distinct, so no
// other mover looks for this key and a compare-and-swap on an empty key is the whole probe -- and the seven words go in as plain stores: the table
// was cleared and nobody else touches that record.  The probe ends after dst_slots steps with the failure word set; it cannot legitimately run out.
__global__ __launch_bounds__(kVmT) void k_vm_rehash(const VmGrowJob *jobs)
{
    const VmGrowJob &j = jobs[blockIdx.y];
    const unsigned long long base = (unsigned long long)blockIdx.x * kVmTile;
    if (base >= j.src_slots) return;
    __shared__ unsigned l_moved;
    if (threadIdx.x == 0) l_moved = 0;
    __syncthreads();
    const int w = threadIdx.x & 7, lead = threadIdx.x & 63 & ~7;         // lead: lane 0 of this group of eight
    const unsigned mask = (unsigned)(j.dst_slots - 1);
    unsigned moved = 0;
    // kVmRehashU records per group at a time: their loads are issued together, then their first compare-and-swaps, so a workgroup has
    // kVmRehashU times the bytes in flight of one record at a time (measured: profiles/r18)
    for (int r0 = 0; r0 < kVmTile * 8 / kVmT; r0 += kVmRehashU) {
        unsigned long long v[kVmRehashU], key[kVmRehashU], got[kVmRehashU];
        unsigned h[kVmRehashU];
        bool mover[kVmRehashU];
#pragma unroll
        for (int u = 0; u < kVmRehashU; u++) {
            const unsigned long long rec = base + (unsigned long long)((r0 + u) * (kVmT / 8)) + (threadIdx.x >> 3);
            v[u] = rec < j.src_slots ? ((const uint64_t *)j.src)[rec * 8 + w] : (w == 0 ? kVmEmpty : 0ull);
        }
#pragma unroll
        for (int u = 0; u < kVmRehashU; u++) {
            key[u] = __shfl(v[u], lead);
            const unsigned long long count = __shfl(v[u], lead + 1);
            mover[u] = w == 0 && key[u] != kVmEmpty && count != 0;
            h[u] = (unsigned)vm_mix(key[u]) & mask;
            got[u] = 0;
        }
#pragma unroll
        for (int u = 0; u < kVmRehashU; u++)
            if (mover[u]) got[u] = atomicCAS((unsigned long long *)&j.dst[h[u]].key, (unsigned long long)kVmEmpty, key[u]);
#pragma unroll
        for (int u = 0; u < kVmRehashU; u++) {
            unsigned slot = kVmNoSlot;
            if (mover[u]) {
                if (got[u] == kVmEmpty) slot = h[u];
                else                                                        // the first slot was taken: the other dst_slots - 1, one by one
                    for (unsigned probe = 0, at = (h[u] + 1) & mask; probe < mask; probe++, at = (at + 1) & mask)
                        if (atomicCAS((unsigned long long *)&j.dst[at].key, (unsigned long long)kVmEmpty, key[u]) == kVmEmpty) { slot = at; break; }
                if (slot == kVmNoSlot) atomicExch(j.res, 1);
                else moved++;
            }
            slot = __shfl(slot, lead);
            if (slot != kVmNoSlot && w != 0) j.dst[slot].w[w - 1] = v[u];
        }
    }
    if (moved) atomicAdd(&l_moved, moved);
    __syncthreads();
    if (threadIdx.x == 0 && l_moved) {
        atomicAdd((unsigned *)(j.dst + j.dst_slots), l_moved);      // the new table's occupancy counter
        atomicAdd(j.res + 1, (int)l_moved);
    }
}

// records with count > 0, in no order, into out[cap]; n counts them all
// the output point of an occupied record as a cloud point (what lmono_voxel_map_read gives)
__device__ inline PtRgb vm_out_point(const VmRec &r, float leaf)
{
    const VmPoint p = vm_point(r, leaf);
    PtRgb o;
    o.x = p.x; o.y = p.y; o.z = p.z; o.bgra = p.bgra;
    return o;
}

__global__ __launch_bounds__(kVmT) void k_vm_compact(const VmRec *rec, unsigned long long slots, VmRec *out, unsigned cap, unsigned *n)
{
    const unsigned long long s = (unsigned long long)blockIdx.x * kVmT + threadIdx.x;
    if (s >= slots) return;
    const VmRec r = rec[s];
    if (!vm_occupied(r)) return;
    const unsigned at = atomicAdd(n, 1u);
    if (at < cap) out[at] = r;
}

// every occupied voxel's output point (vm_point, what lmono_voxel_map_read gives) into out, in any order; n counts them, cap bounds the writes:
// a map as the input cloud of another stage (the ICP's target, the surface normals)
__global__ __launch_bounds__(kVmT) void k_vm_points_unordered(const VmRec *rec, unsigned long long slots, float leaf, PtRgb *out, unsigned cap, unsigned *n)
{
    const unsigned long long s = (unsigned long long)blockIdx.x * kVmT + threadIdx.x;
    if (s >= slots) return;
    const VmRec r = rec[s];
    if (!vm_occupied(r)) return;
    const unsigned at = atomicAdd(n, 1u);
    if (at < cap) out[at] = vm_out_point(r, leaf);
}

// ---- compose: whole voxel maps, each under a rigid transform, folded into one destination ----
// The sources' occupied records (k_vm_compact, no order) are the input; blockIdx.y = source.  The plain form -- one probe and one entry per record --
// because a map's records are one per cell already: at comparable leaves about one source voxel lands in a destination voxel per tile, so a
// workgroup table would find nothing to merge (scripts/voxel_compose_bench.py reports the ratio).  Entries and addends are 64-bit: count * offset
// passes 32 bits at a count above 65536.
struct VmMoveEnt { unsigned long long slot, w[7]; };    // slot: kVmNoSlot when the voxel is rejected or found no slot
struct VmMoveSrc {
    const VmRec *rec;                      // the source's occupied records
    unsigned n;
    float leaf;
    long long ent_off;                     // this source's part of the call's entries
    double T[12];
};
static_assert(sizeof(VmMoveEnt) == 64, "compose entry layout");

// stat: [0] voxels moved, [1] voxels rejected, [2] points moved, [3] points rejected.  j: the destination (pts, n, ent, tile_n unused);
// j.res as in k_vm_find: [0] failure word, [3] occupancy after the call
__global__ __launch_bounds__(kVmT) void k_vm_move_find(const VmJob j, const VmMoveSrc *srcs, VmMoveEnt *ent, unsigned long long *stat)
{
    const VmMoveSrc &s = srcs[blockIdx.y];
    const unsigned base = blockIdx.x * kVmTile;
    if (base >= s.n) return;
    __shared__ unsigned l_claims, l_vrej;
    __shared__ unsigned long long l_pts, l_prej;
    const int tid = threadIdx.x;
    if (tid == 0) { l_claims = 0; l_vrej = 0; l_pts = 0; l_prej = 0; }
    __syncthreads();
    for (int r = 0; r < kVmTile / kVmT; r++) {
        const unsigned i = base + r * kVmT + tid;
        if (i >= s.n) continue;
        const VmRec rec = s.rec[i];
        uint64_t key = kVmEmpty, add[7] = { 0, 0, 0, 0, 0, 0, 0 };
        const bool ok = vm_move(rec, s.leaf, s.T, j.inv, key, add);
        VmMoveEnt e;
        e.slot = ok ? vm_find_or_claim(j, key, &l_claims) : kVmNoSlot;
        for (int w = 0; w < 7; w++) e.w[w] = add[w];
        ent[s.ent_off + i] = e;
        if (ok) atomicAdd(&l_pts, (unsigned long long)rec.w[0]);
        else { atomicAdd(&l_vrej, 1u); atomicAdd(&l_prej, (unsigned long long)rec.w[0]); }
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned left = s.n - base, in_tile = left < kVmTile ? left : kVmTile;
        // one block of tickets for the slots this workgroup claimed: a ticket >= max_voxels refuses the call
        if (l_claims && atomicAdd(j.occ, l_claims) + l_claims > j.max_voxels) atomicExch(j.res, 1);
        if (in_tile - l_vrej) atomicAdd(stat + 0, (unsigned long long)(in_tile - l_vrej));
        if (l_vrej) atomicAdd(stat + 1, (unsigned long long)l_vrej);
        if (l_pts) atomicAdd(stat + 2, l_pts);
        if (l_prej) atomicAdd(stat + 3, l_prej);
    }
}

__global__ __launch_bounds__(kVmT) void k_vm_move_accum(const VmJob j, const VmMoveSrc *srcs, const VmMoveEnt *ent)
{
    const VmMoveSrc &s = srcs[blockIdx.y];
    const unsigned base = blockIdx.x * kVmTile;
    if (base >= s.n) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) j.res[3] = (int)*j.occ;      // every source's first workgroup writes the same value
    if (j.res[0] != 0) return;                 // the sources do not fit: nothing of the call enters the map
    const unsigned left = s.n - base, n = left < kVmTile ? left : kVmTile;
    const int w = threadIdx.x & 7;
    for (unsigned e = threadIdx.x >> 3; e < n; e += kVmT / 8) {
        const VmMoveEnt *en = ent + s.ent_off + base + e;
        const unsigned long long slot = en->slot;
        if (slot == kVmNoSlot || w == 0) continue;      // word 0 of a record is its key
        const unsigned long long v = en->w[w - 1];
        if (v) atomicAdd((unsigned long long *)&j.rec[slot].w[w - 1], v);
    }
}

__global__ __launch_bounds__(kVmT) void k_vm_finish(const VmRec *rec, unsigned n, float leaf, PtRgb *out)
{
    const unsigned i = blockIdx.x * kVmT + threadIdx.x;
    if (i >= n) return;
    out[i] = vm_out_point(rec[i], leaf);
}

} // namespace lmono
