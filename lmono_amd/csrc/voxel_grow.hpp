// voxel_grow.hpp -- the two pure functions of a voxel map that changes size: how many slots a table for max_voxels voxels has,
// and which capacity a growing map stands at after a call.  One text for the C ABI (voxel_map_abi.hip) and for the CPU program
// host/voxel_grow_test.cpp; no HIP, no GPU.
#pragma once
#include <cstdint>

namespace lmono {

constexpr int64_t kVmMaxVoxels = (int64_t)1 << 30;          // largest max_voxels of a map, and largest growth limit

// slots of the table of a map of max_voxels voxels: the power of two >= 2 * max_voxels, at least 2 (load <= 1/2)
inline uint64_t vm_slots(int64_t max_voxels)
{
    uint64_t slots = 2;
    while (slots < 2 * (uint64_t)max_voxels) slots <<= 1;
    return slots;
}

// one growth step of a map at max_voxels under the limit (0: growth off): min(limit, 2 * max_voxels), or max_voxels itself when it cannot grow
inline int64_t vm_grow_step(int64_t max_voxels, int64_t limit)
{
    if (limit <= max_voxels) return max_voxels;
    return 2 * max_voxels < limit ? 2 * max_voxels : limit;
}

// The capacity after a call that needs `voxels` voxels in all (those in the map and the new ones), on a map at max_voxels.  Exactly max_voxels
// voxels fit, and a refused call grows the map by one step and is repeated, so this is the smallest of m, step(m), step(step(m)), ... that is
// >= voxels, and the last of them (the limit) when none is: that call is refused there.
inline int64_t vm_grow_capacity(int64_t max_voxels, int64_t limit, int64_t voxels)
{
    while (max_voxels < voxels) {
        const int64_t next = vm_grow_step(max_voxels, limit);
        if (next == max_voxels) break;
        max_voxels = next;
    }
    return max_voxels;
}

} // namespace lmono
