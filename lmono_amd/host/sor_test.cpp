// lmono_amd/host/sor_test.cpp -- the statistical outlier removal on the host: the whole definition by brute force over
// csrc/sor.hpp, the text the kernels run; no grid, no GPU library.
//   sor_test <points.bin> <mean_k> <stddev_mul> <cell> <max_rings>
// points.bin: [n] records x y z float32 + bgra uint32.  Prints
//   stats <points in> <rejected> <isolated> <M> <kept> <A> <Bhi> <Blo>
//   threshold <mean> <sqrt(var)> <thr>            (fp64 bit patterns, hex)
// then per input point "<keep> <v, hex>" (v = ffffffff: rejected or isolated).
#include "../csrc/sor.hpp"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace lmono;

int main(int argc, char **argv)
{
    if (argc < 6) { std::fprintf(stderr, "usage: sor_test <points.bin> <mean_k> <stddev_mul> <cell> <max_rings>\n"); return 2; }
    const int k = std::atoi(argv[2]), rings = std::atoi(argv[5]);
    const double mul = std::strtod(argv[3], nullptr);
    const float h = std::strtof(argv[4], nullptr);
    if (k < 1 || k > kSorMaxK || rings < 1 || rings > kSorMaxRings || !std::isfinite(mul) || !std::isfinite(h) || !(h > 0.0f) || !(sor_rho(rings, h) <= kSorMaxRho)) {
        std::fprintf(stderr, "sor_test: mean_k in 1 .. 128, stddev_mul finite, cell finite and > 0, max_rings in 1 .. 64, (max_rings - 0.25) cell <= 256\n");
        return 2;
    }
    const float inv = 1.0f / h, rho2 = sor_rho2(rings, h);
    std::vector<VmPoint> pts;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
        VmPoint p;
        while (std::fread(&p, sizeof p, 1, f) == 1) pts.push_back(p);
        std::fclose(f);
    }
    const size_t n = pts.size();
    std::vector<char> valid(n);
    std::vector<uint32_t> v(n, kSorNoScore);
    uint64_t rejected = 0, isolated = 0, M = 0, A = 0, Bhi = 0, Blo = 0, kept = 0;
    for (size_t i = 0; i < n; i++) {
        uint64_t key;
        int c[3];
        valid[i] = sor_cell(pts[i].x, pts[i].y, pts[i].z, inv, key, c);
        if (!valid[i]) rejected++;
    }
    std::vector<float> d;
    for (size_t i = 0; i < n; i++) {
        if (!valid[i]) continue;
        d.clear();
        for (size_t j = 0; j < n; j++) {
            if (j == i || !valid[j]) continue;
            const float d2 = sor_d2(pts[i].x, pts[i].y, pts[i].z, pts[j].x, pts[j].y, pts[j].z);
            if (d2 <= rho2) d.push_back(d2);
        }
        if (d.size() < (size_t)k) { isolated++; continue; }
        std::nth_element(d.begin(), d.begin() + (k - 1), d.end());
        uint64_t S = 0;
        for (int q = 0; q < k; q++) S += sor_u(d[(size_t)q]);
        v[i] = sor_v(S);
        uint64_t a, bhi, blo;
        sor_terms(v[i], a, bhi, blo);
        M++; A += a; Bhi += bhi; Blo += blo;
    }
    double mean, sd;
    const double thr = sor_threshold(M, A, Bhi, Blo, mul, mean, sd);
    for (size_t i = 0; i < n; i++) kept += sor_keep(v[i], thr) ? 1 : 0;
    uint64_t b[3];
    std::memcpy(&b[0], &mean, 8); std::memcpy(&b[1], &sd, 8); std::memcpy(&b[2], &thr, 8);
    std::printf("stats %zu %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", n, rejected, isolated, M, kept, A, Bhi, Blo);
    std::printf("threshold %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", b[0], b[1], b[2]);
    for (size_t i = 0; i < n; i++) std::printf("%d %08x\n", sor_keep(v[i], thr) ? 1 : 0, v[i]);
    return 0;
}
