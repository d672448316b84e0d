// lmono_amd/host/voxel_grow_test.cpp -- the size arithmetic of a voxel map that grows on the host: the header the C ABI
// includes, no GPU library.
//   voxel_grow_test slots M...            one line "M SLOTS" per max_voxels M: the slots of that map's table
//   voxel_grow_test grow M0 LIMIT V...    one line "V CAPACITY" per call: a map created at M0 with growth limit LIMIT (0: fixed) takes calls after
//                                          which it would hold V voxels in all; CAPACITY is its max_voxels after that call (a call that does not fit
//                                          at the limit is refused there, and the capacity stays at the limit)
#include "../csrc/voxel_grow.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace lmono;

static bool number(const char *s, int64_t lo, int64_t &v)
{
    char *end = nullptr;
    v = std::strtoll(s, &end, 10);
    return end && end != s && *end == 0 && v >= lo && v <= kVmMaxVoxels;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && std::strcmp(argv[1], "slots") == 0) {
        for (int a = 2; a < argc; a++) {
            int64_t m;
            if (!number(argv[a], 1, m)) { std::fprintf(stderr, "voxel_grow_test: max_voxels must be in 1 .. 2^30\n"); return 2; }
            std::printf("%lld %llu\n", (long long)m, (unsigned long long)vm_slots(m));
        }
        return 0;
    }
    if (argc >= 4 && std::strcmp(argv[1], "grow") == 0) {
        int64_t cap, limit;
        if (!number(argv[2], 1, cap) || !number(argv[3], 0, limit) || (limit != 0 && limit < cap)) {
            std::fprintf(stderr, "voxel_grow_test: M0 in 1 .. 2^30, LIMIT 0 or in M0 .. 2^30\n");
            return 2;
        }
        for (int a = 4; a < argc; a++) {
            int64_t v;
            if (!number(argv[a], 0, v)) { std::fprintf(stderr, "voxel_grow_test: voxel counts must be in 0 .. 2^30\n"); return 2; }
            cap = vm_grow_capacity(cap, limit, v);
            std::printf("%lld %lld\n", (long long)v, (long long)cap);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: voxel_grow_test slots M... | voxel_grow_test grow M0 LIMIT V...\n");
    return 2;
}
