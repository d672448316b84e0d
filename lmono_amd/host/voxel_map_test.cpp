// lmono_amd/host/voxel_map_test.cpp -- the voxel-grid colour map on the host: the arithmetic of csrc/voxel_map.hpp,
// the text the kernels run, over a std::map; no GPU library.
//   voxel_map_test <points.bin> <leaf>
// points.bin: [n] records x y z float32 + bgra uint32.  Prints "rejected <n>", then per voxel in ascending key order
//   <key> <count> <sx> <sy> <sz> <sr> <sg> <sb> <x y z as float32 bit patterns, hex> <bgra, hex>
#include "../csrc/voxel_map.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

using namespace lmono;

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: voxel_map_test <points.bin> <leaf>\n"); return 2; }
    const float leaf = std::strtof(argv[2], nullptr);
    if (!std::isfinite(leaf) || !(leaf > 0.0f)) { std::fprintf(stderr, "voxel_map_test: leaf must be finite and > 0\n"); return 2; }
    const float inv = 1.0f / leaf;
    std::vector<VmPoint> pts;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
        VmPoint p;
        while (std::fread(&p, sizeof p, 1, f) == 1) pts.push_back(p);
        std::fclose(f);
    }
    std::map<uint64_t, VmRec> table;
    uint64_t rejected = 0;
    for (const VmPoint &p : pts) {
        uint64_t key;
        int q[3];
        if (!vm_cell(p.x, p.y, p.z, inv, key, q)) { rejected++; continue; }
        auto it = table.find(key);
        if (it == table.end()) {
            VmRec r{};
            r.key = key;
            it = table.emplace(key, r).first;
        }
        VmRec &r = it->second;
        r.w[0] += 1;
        for (int a = 0; a < 3; a++) r.w[1 + a] += (uint64_t)q[a];
        r.w[4] += p.bgra >> 16 & 255u; r.w[5] += p.bgra >> 8 & 255u; r.w[6] += p.bgra & 255u;
    }
    std::printf("rejected %" PRIu64 "\n", rejected);
    for (const auto &kv : table) {
        const VmRec &r = kv.second;
        const VmPoint o = vm_point(r, leaf);
        uint32_t b[3];
        std::memcpy(&b[0], &o.x, 4); std::memcpy(&b[1], &o.y, 4); std::memcpy(&b[2], &o.z, 4);
        std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %08x %08x %08x %08x\n", r.key, r.w[0], r.w[1], r.w[2],
                    r.w[3], r.w[4], r.w[5], r.w[6], b[0], b[1], b[2], o.bgra);
    }
    return 0;
}
