// lmono_amd/host/normals_test.cpp -- the surface normals on the host: the whole definition by brute force over all pairs with
// csrc/normals.hpp, the text the kernels run; no grid, no GPU library.
//   normals_test <cloud.bin> <radius> <min_neighbours> <cell> <max_rings> [vx vy vz]
// cloud.bin: [n] records x y z float32 + bgra uint32.  v: the viewpoint (default none).  Prints
//   stats <points in> <rejected> <with a normal> <without> <sum of the counts> <largest count> 0 0
//   offdiag <largest |off-diagonal| left by the Jacobi sweeps over all points, %g>
// then per point "<nx> <ny> <nz> <curvature> <count>" (float32 bit patterns, hex; the count decimal).
#include "../csrc/normals.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace lmono;

static uint32_t bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }

int main(int argc, char **argv)
{
    if (argc != 6 && argc != 9) { std::fprintf(stderr, "usage: normals_test <cloud.bin> <radius> <min_neighbours> <cell> <max_rings> [vx vy vz]\n"); return 2; }
    const float r = std::strtof(argv[2], nullptr), h = std::strtof(argv[4], nullptr);
    const int min_nb = std::atoi(argv[3]), rings = std::atoi(argv[5]);
    if (!nrm_params_ok(r, min_nb, h, rings)) {
        std::fprintf(stderr, "normals_test: 0 < radius <= 4, min_neighbours >= 3, cell > 0, max_rings in 1 .. 64, (max_rings - 0.25) cell >= radius\n");
        return 2;
    }
    float vp[3] = { 0.0f, 0.0f, 0.0f };
    const bool has_vp = argc == 9;
    if (has_vp) for (int a = 0; a < 3; a++) vp[a] = std::strtof(argv[6 + a], nullptr);
    std::vector<VmPoint> pts;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
        VmPoint p;
        while (std::fread(&p, sizeof p, 1, f) == 1) pts.push_back(p);
        std::fclose(f);
    }
    const size_t n = pts.size();
    if ((long long)n > kNrmMaxPoints) { std::fprintf(stderr, "normals_test: more than 2^26 points\n"); return 2; }
    const float inv = 1.0f / h, r2 = r * r;

    // validity, origin, span
    std::vector<char> ok(n, 0);
    uint32_t kmin[3] = { 0xffffffffu, 0xffffffffu, 0xffffffffu }, kmax[3] = { 0, 0, 0 };
    uint64_t key;
    int c[3];
    for (size_t i = 0; i < n; i++) {
        ok[i] = sor_cell(pts[i].x, pts[i].y, pts[i].z, inv, key, c);
        if (!ok[i]) continue;
        const uint32_t k[3] = { icp_ord(pts[i].x), icp_ord(pts[i].y), icp_ord(pts[i].z) };
        for (int a = 0; a < 3; a++) { if (k[a] < kmin[a]) kmin[a] = k[a]; if (k[a] > kmax[a]) kmax[a] = k[a]; }
    }
    float o[3];
    for (int a = 0; a < 3; a++) o[a] = kmin[a] <= kmax[a] ? icp_origin(icp_unord(kmin[a]), icp_unord(kmax[a])) : 0.0f;
    std::vector<int> iw(3 * n, 0);
    int64_t stats[8] = { (int64_t)n, 0, 0, 0, 0, 0, 0, 0 };
    for (size_t i = 0; i < n; i++) {
        ok[i] = ok[i] && icp_in_span(pts[i].x - o[0]) && icp_in_span(pts[i].y - o[1]) && icp_in_span(pts[i].z - o[2]);
        if (!ok[i]) { stats[1]++; continue; }
        iw[3 * i] = nrm_fix(pts[i].x - o[0]); iw[3 * i + 1] = nrm_fix(pts[i].y - o[1]); iw[3 * i + 2] = nrm_fix(pts[i].z - o[2]);
    }
    std::vector<NrmRecord> rec(n, nrm_no_normal());
    std::vector<uint32_t> count(n, 0);
    double off = 0.0;
    for (size_t i = 0; i < n; i++) {
        if (!ok[i]) continue;
        NrmSums s;
        std::memset(&s, 0, sizeof s);
        for (size_t j = 0; j < n; j++) {
            if (!ok[j] || !(sor_d2(pts[i].x, pts[i].y, pts[i].z, pts[j].x, pts[j].y, pts[j].z) <= r2)) continue;
            nrm_add(&iw[3 * i], &iw[3 * j], s);
        }
        count[i] = (uint32_t)s.N;
        stats[4] += s.N;
        if (s.N > stats[5]) stats[5] = s.N;
        if (s.N < min_nb) { stats[3]++; continue; }
        stats[2]++;
        double swept[9];
        rec[i] = nrm_solve(s, pts[i].x, pts[i].y, pts[i].z, has_vp ? vp : nullptr, swept);
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) if (a != b && std::fabs(swept[3 * a + b]) > off) off = std::fabs(swept[3 * a + b]);
    }
    std::printf("stats");
    for (int k = 0; k < 8; k++) std::printf(" %" PRId64, stats[k]);
    std::printf("\noffdiag %g\n", off);
    for (size_t i = 0; i < n; i++) std::printf("%08x %08x %08x %08x %u\n", bits(rec[i].nx), bits(rec[i].ny), bits(rec[i].nz), bits(rec[i].curvature), count[i]);
    return 0;
}
