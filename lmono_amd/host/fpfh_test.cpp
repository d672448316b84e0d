// lmono_amd/host/fpfh_test.cpp -- the FPFH descriptors on the host: the whole definition by brute force over all pairs with
// csrc/fpfh.hpp, the text the kernels run; no grid, no GPU library.
//   fpfh_test <cloud.bin> <normals.bin> <keypoints.bin> <radius> <cell> <max_rings>
// cloud.bin: [n] records x y z float32 + bgra uint32.  normals.bin: [n] records nx ny nz curvature float32 (NaN: no normal).  keypoints.bin:
// [m][3] float32.  Prints
//   stats <keypoints in> <with a descriptor> <without> <points with an SPFH> <sum of the pair counts> <largest> <sum of the contributing points> <largest>
// then per keypoint the 33 floats of its descriptor (bit patterns, hex), the contributing points and the flag (decimal).
#include "../csrc/fpfh.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace lmono;

static uint32_t bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }

template <typename T> static bool read_all(const char *path, std::vector<T> &out)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); return false; }
    T v;
    while (std::fread(&v, sizeof v, 1, f) == 1) out.push_back(v);
    std::fclose(f);
    return true;
}

struct Kp { float x, y, z; };

int main(int argc, char **argv)
{
    if (argc != 7) { std::fprintf(stderr, "usage: fpfh_test <cloud.bin> <normals.bin> <keypoints.bin> <radius> <cell> <max_rings>\n"); return 2; }
    const float r = std::strtof(argv[4], nullptr), h = std::strtof(argv[5], nullptr);
    const int rings = std::atoi(argv[6]);
    if (!fpfh_params_ok(r, h, rings)) { std::fprintf(stderr, "fpfh_test: 0 < radius <= 4, cell > 0, max_rings in 1 .. 64, (max_rings - 0.25) cell >= radius\n"); return 2; }
    std::vector<VmPoint> pts;
    std::vector<NrmRecord> rec;
    std::vector<Kp> kp;
    if (!read_all(argv[1], pts) || !read_all(argv[2], rec) || !read_all(argv[3], kp)) return 1;
    const size_t n = pts.size(), m = kp.size();
    if (rec.size() != n || (long long)n > kFpfhMaxPoints || m > (size_t)kFpfhMaxKeypoints) { std::fprintf(stderr, "fpfh_test: one record per point, at most 2^26 points and 4096 keypoints\n"); return 2; }
    const float inv = 1.0f / h, r2 = r * r;

    // validity, origin, span, normal
    std::vector<char> has(n, 0);
    uint32_t kmin[3] = { 0xffffffffu, 0xffffffffu, 0xffffffffu }, kmax[3] = { 0, 0, 0 };
    uint64_t key;
    int c[3];
    for (size_t i = 0; i < n; i++) {
        has[i] = sor_cell(pts[i].x, pts[i].y, pts[i].z, inv, key, c);
        if (!has[i]) continue;
        const uint32_t k[3] = { icp_ord(pts[i].x), icp_ord(pts[i].y), icp_ord(pts[i].z) };
        for (int a = 0; a < 3; a++) { if (k[a] < kmin[a]) kmin[a] = k[a]; if (k[a] > kmax[a]) kmax[a] = k[a]; }
    }
    float o[3];
    for (int a = 0; a < 3; a++) o[a] = kmin[a] <= kmax[a] ? icp_origin(icp_unord(kmin[a]), icp_unord(kmax[a])) : 0.0f;
    for (size_t i = 0; i < n; i++)
        has[i] = has[i] && icp_in_span(pts[i].x - o[0]) && icp_in_span(pts[i].y - o[1]) && icp_in_span(pts[i].z - o[2]) && fpfh_has_normal(rec[i].nx);

    // needed points
    std::vector<char> usable(m, 0), needed(n, 0);
    for (size_t k = 0; k < m; k++) {
        usable[k] = sor_cell(kp[k].x, kp[k].y, kp[k].z, inv, key, c);
        if (!usable[k]) continue;
        for (size_t j = 0; j < n; j++)
            if (has[j] && sor_d2(kp[k].x, kp[k].y, kp[k].z, pts[j].x, pts[j].y, pts[j].z) <= r2) needed[j] = 1;
    }
    int64_t stats[8] = { (int64_t)m, 0, 0, 0, 0, 0, 0, 0 };
    std::vector<unsigned> spfh(n * (size_t)kFpfhRow, 0u);
    for (size_t i = 0; i < n; i++) {
        if (!needed[i]) continue;
        unsigned *row = &spfh[i * kFpfhRow];
        for (size_t j = 0; j < n; j++) {
            if (!has[j]) continue;
            const float d2 = sor_d2(pts[i].x, pts[i].y, pts[i].z, pts[j].x, pts[j].y, pts[j].z);
            if (!(d2 > 0.0f && d2 <= r2)) continue;
            int b[3];
            if (!fpfh_pair(pts[i].x, pts[i].y, pts[i].z, rec[i].nx, rec[i].ny, rec[i].nz, pts[j].x, pts[j].y, pts[j].z, rec[j].nx, rec[j].ny, rec[j].nz, b)) continue;
            row[b[0]]++; row[kFpfhBins + b[1]]++; row[2 * kFpfhBins + b[2]]++; row[kFpfhDim]++;
        }
        stats[3]++; stats[4] += row[kFpfhDim];
        if ((int64_t)row[kFpfhDim] > stats[5]) stats[5] = row[kFpfhDim];
    }
    std::vector<float> desc(m * (size_t)kFpfhDim, 0.0f);
    std::vector<unsigned> nb(m, 0u);
    for (size_t k = 0; k < m; k++) {
        uint64_t hi[kFpfhDim], lo[kFpfhDim];
        for (int b = 0; b < kFpfhDim; b++) { hi[b] = 0; lo[b] = 0; }
        for (size_t j = 0; usable[k] && j < n; j++) {
            if (!needed[j]) continue;
            const float d2 = sor_d2(kp[k].x, kp[k].y, kp[k].z, pts[j].x, pts[j].y, pts[j].z);
            const unsigned *row = &spfh[j * kFpfhRow];
            if (!(d2 <= r2) || row[kFpfhDim] == 0) continue;
            const uint64_t W = fpfh_weight(d2, row[kFpfhDim]);
            nb[k]++;
            for (int b = 0; b < kFpfhDim; b++) fpfh_add(W, row[b], hi[b], lo[b]);
        }
        stats[nb[k] ? 1 : 2]++; stats[6] += nb[k];
        if ((int64_t)nb[k] > stats[7]) stats[7] = nb[k];
        if (!nb[k]) continue;
        double v[kFpfhDim];
        for (int b = 0; b < kFpfhDim; b++) v[b] = fpfh_value(hi[b], lo[b]);
        for (int b = 0; b < kFpfhDim; b++) desc[k * kFpfhDim + b] = fpfh_scale(v[b], fpfh_total(v + (b / kFpfhBins) * kFpfhBins));
    }
    std::printf("stats");
    for (int k = 0; k < 8; k++) std::printf(" %" PRId64, stats[k]);
    std::printf("\n");
    for (size_t k = 0; k < m; k++) {
        for (int b = 0; b < kFpfhDim; b++) std::printf("%08x ", bits(desc[k * kFpfhDim + b]));
        std::printf("%u %u\n", nb[k], nb[k] ? 1u : 0u);
    }
    return 0;
}
