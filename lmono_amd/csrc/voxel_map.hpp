// voxel_map.hpp -- the arithmetic of the voxel-grid colour map: cell, in-cell offset, key, hash and output point.
// One text for the kernels (voxel_map.hip) and for the CPU programs (host/voxel_map_test.cpp, host/voxel_compose_test.cpp); every float operation is a single IEEE
// operation (build with -ffp-contract=off).  The filter is the pcl::VoxelGrid<pcl::PointXYZRGB> that MapBuilder::processMapping
// left commented out (Map_Builder.cc:82-98); its definition here is this project's own and differs from PCL's in three ways:
// in-cell offsets are 16-bit fixed point and summed as integers, cells are 64-bit keys with no bounding box (and no int32 limit on the
// cell count), and the output order is fixed by the key.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LMONO_VM_HD __host__ __device__ inline
#else
#define LMONO_VM_HD inline
#endif

namespace lmono {

constexpr uint64_t kVmEmpty = ~0ull;             // keys are below 2^63: the empty-slot mark is free
constexpr float kVmCellLimit = 1048576.0f;       // cells -2^20 .. 2^20 - 1 per axis

// One table slot: 64 B, exact integers only.  w[0] = count, w[1..3] = sum of offsets (x y z), w[4..6] = sum of colour bytes (r g b)
struct VmRec { uint64_t key; uint64_t w[7]; };
struct VmPoint { float x, y, z; uint32_t bgra; };

// one axis: cell index and 16-bit offset of coordinate x at inv = 1.0f / leaf; false when the point is rejected (NaN, inf, |cell| >= 2^20)
LMONO_VM_HD bool vm_axis(float x, float inv, int &i, int &q)
{
    const float t = x * inv;
    if (!(t >= -kVmCellLimit && t < kVmCellLimit)) return false;   // before any float -> int cast
    const float c = floorf(t);
    i = (int)c;
    const float f = t - c;                        // 0 <= f <= 1: x = -1e-9f gives exactly 1.0f
    const int v = (int)(f * 65536.0f);
    q = v < 65535 ? v : 65535;
    return true;
}

LMONO_VM_HD uint64_t vm_key(int ix, int iy, int iz)
{
    return (uint64_t)(iz + (1 << 20)) << 42 | (uint64_t)(iy + (1 << 20)) << 21 | (uint64_t)(ix + (1 << 20));
}

// key and offsets q[3] of a point; false when it is rejected
LMONO_VM_HD bool vm_cell(float x, float y, float z, float inv, uint64_t &key, int q[3])
{
    int ix, iy, iz;
    if (!vm_axis(x, inv, ix, q[0]) || !vm_axis(y, inv, iy, q[1]) || !vm_axis(z, inv, iz, q[2])) return false;
    key = vm_key(ix, iy, iz);
    return true;
}

// 64-bit mix of the key (the finaliser of splitmix64); the table takes its low bits, a workgroup's LDS table the high ones
LMONO_VM_HD uint64_t vm_mix(uint64_t k)
{
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return k;
}

// a table slot that holds a voxel: claimed, and by a call that was not refused (a refused call's claims stay with count 0, unseen)
LMONO_VM_HD bool vm_occupied(const VmRec &r) { return r.key != kVmEmpty && r.w[0] != 0; }

// exact (every conversion and the sum under the division are exact, so the result is the correctly rounded chain of the formula) while
// s + count / 2 < 2^53; s <= 65535 * count, so while a voxel's count stays below 2^36 -- composed maps (below) reach counts inserts never do
LMONO_VM_HD float vm_axis_out(int i, uint64_t s, uint64_t count, float leaf)
{
    return (float)(((double)i + ((double)s + 0.5 * (double)count) / (65536.0 * (double)count)) * (double)leaf);
}

// the output point of a voxel (count > 0): mean offset at the middle of its 2^-16 step, colour bytes truncated, alpha 255
LMONO_VM_HD VmPoint vm_point(const VmRec &r, float leaf)
{
    const int ix = (int)(r.key & 0x1fffff) - (1 << 20), iy = (int)(r.key >> 21 & 0x1fffff) - (1 << 20), iz = (int)(r.key >> 42 & 0x1fffff) - (1 << 20);
    const uint64_t n = r.w[0];
    VmPoint p;
    p.x = vm_axis_out(ix, r.w[1], n, leaf);
    p.y = vm_axis_out(iy, r.w[2], n, leaf);
    p.z = vm_axis_out(iz, r.w[3], n, leaf);
    p.bgra = (uint32_t)(r.w[6] / n) | (uint32_t)(r.w[5] / n) << 8 | (uint32_t)(r.w[4] / n) << 16 | 0xff000000u;
    return p;
}

// ---- composing voxel maps under rigid transforms ----
// One coordinate of T * p, T a row of a row-major 3 x 4 fp64 transform: fp64 products and sums in exactly this order, one cast
LMONO_VM_HD float vm_move_axis(const double *row, const VmPoint &p)
{
    return (float)(((row[0] * (double)p.x + row[1] * (double)p.y) + row[2] * (double)p.z) + row[3]);
}

// A voxel r (count c > 0) of a map with leaf leaf_src, moved by T into a map with inv = 1.0f / leaf: its output point goes where a point would, with
// weight c.  add[0] = c, add[1..3] = c * q, add[4..6] = r's own colour sums (not c * the truncated mean: colour sums are conserved exactly).
// false when the moved point is rejected (the voxel and its c points are counted, nothing is added).  The products pass 32 bits at c > 65536.
LMONO_VM_HD bool vm_move(const VmRec &r, float leaf_src, const double *T, float inv, uint64_t &key, uint64_t add[7])
{
    const VmPoint p = vm_point(r, leaf_src);
    int q[3];
    if (!vm_cell(vm_move_axis(T, p), vm_move_axis(T + 4, p), vm_move_axis(T + 8, p), inv, key, q)) return false;
    add[0] = r.w[0];
    for (int a = 0; a < 3; a++) { add[1 + a] = r.w[0] * (uint64_t)q[a]; add[4 + a] = r.w[4 + a]; }
    return true;
}

} // namespace lmono
