// lmono_amd/host/voxel_compose_test.cpp -- composing voxel maps under rigid transforms on the host: the arithmetic of
// csrc/voxel_map.hpp, the text the kernels run, over std::map; no GPU library.
//   voxel_compose_test <leaf_dst> <transforms.bin> <points0.bin> <leaf0> [<points1.bin> <leaf1> ...]
// transforms.bin: [n][12] float64, row-major 3 x 4, one per source.  pointsK.bin: [n] records x y z float32 + bgra uint32, inserted into a
// source map of leafK.  The sources are composed, in the order given, into an empty map of leaf_dst.  Prints "rejected <voxels> <points>",
// then per voxel of the composed map, in ascending key order, the line of voxel_map_test:
//   <key> <count> <sx> <sy> <sz> <sr> <sg> <sb> <x y z as float32 bit patterns, hex> <bgra, hex>
#include "../csrc/voxel_map.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

using namespace lmono;

typedef std::map<uint64_t, VmRec> Table;

static VmRec &slot_of(Table &t, uint64_t key)
{
    auto it = t.find(key);
    if (it == t.end()) {
        VmRec r{};
        r.key = key;
        it = t.emplace(key, r).first;
    }
    return it->second;
}

static bool leaf_ok(float leaf) { return std::isfinite(leaf) && leaf > 0.0f; }

int main(int argc, char **argv)
{
    if (argc < 5 || (argc - 3) % 2 != 0) { std::fprintf(stderr, "usage: voxel_compose_test <leaf_dst> <transforms.bin> <points.bin> <leaf> [...]\n"); return 2; }
    const float leaf_dst = std::strtof(argv[1], nullptr);
    if (!leaf_ok(leaf_dst)) { std::fprintf(stderr, "voxel_compose_test: leaf must be finite and > 0\n"); return 2; }
    const int n_src = (argc - 3) / 2;
    std::vector<double> T((size_t)n_src * 12);
    {
        FILE *f = std::fopen(argv[2], "rb");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
        const size_t got = std::fread(T.data(), sizeof(double), T.size(), f);
        std::fclose(f);
        if (got != T.size()) { std::fprintf(stderr, "%s: fewer than %d transforms\n", argv[2], n_src); return 1; }
    }
    Table dst;
    uint64_t vox_rejected = 0, pts_rejected = 0;
    for (int s = 0; s < n_src; s++) {
        const float leaf = std::strtof(argv[4 + 2 * s], nullptr);
        if (!leaf_ok(leaf)) { std::fprintf(stderr, "voxel_compose_test: leaf must be finite and > 0\n"); return 2; }
        FILE *f = std::fopen(argv[3 + 2 * s], "rb");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[3 + 2 * s]); return 1; }
        Table src;
        VmPoint p;
        while (std::fread(&p, sizeof p, 1, f) == 1) {
            uint64_t key;
            int q[3];
            if (!vm_cell(p.x, p.y, p.z, 1.0f / leaf, key, q)) continue;
            VmRec &r = slot_of(src, key);
            r.w[0] += 1;
            for (int a = 0; a < 3; a++) r.w[1 + a] += (uint64_t)q[a];
            r.w[4] += p.bgra >> 16 & 255u; r.w[5] += p.bgra >> 8 & 255u; r.w[6] += p.bgra & 255u;
        }
        std::fclose(f);
        for (const auto &kv : src) {
            uint64_t key, add[7];
            if (!vm_move(kv.second, leaf, &T[(size_t)s * 12], 1.0f / leaf_dst, key, add)) { vox_rejected++; pts_rejected += kv.second.w[0]; continue; }
            VmRec &r = slot_of(dst, key);
            for (int w = 0; w < 7; w++) r.w[w] += add[w];
        }
    }
    std::printf("rejected %" PRIu64 " %" PRIu64 "\n", vox_rejected, pts_rejected);
    for (const auto &kv : dst) {
        const VmRec &r = kv.second;
        const VmPoint o = vm_point(r, leaf_dst);
        uint32_t b[3];
        std::memcpy(&b[0], &o.x, 4); std::memcpy(&b[1], &o.y, 4); std::memcpy(&b[2], &o.z, 4);
        std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %08x %08x %08x %08x\n", r.key, r.w[0], r.w[1], r.w[2],
                    r.w[3], r.w[4], r.w[5], r.w[6], b[0], b[1], b[2], o.bgra);
    }
    return 0;
}
