// lmono_amd/host/icp_test.cpp -- the point-to-point ICP on the host: the whole definition by brute force over all pairs with
// csrc/icp.hpp, the text the kernels run; no grid, no GPU library.
//   icp_test <target.bin> <source.bin> <max_corr> <max_iter> <eps> <mse_eps> <cell> <max_rings> [g0 .. g11]
// *.bin: [n] records x y z float32 + bgra uint32.  g: the guess, row-major 3 x 4 (default identity).  Prints
//   transform <12 fp64 bit patterns, hex>
//   stats <source points> <not usable> <target points> <rejected> <iterations> <status> <N> <E>
//   offdiag <largest |off-diagonal| left by the Jacobi sweeps over all iterations, %g>
//   history <k>, then k lines "<N> <E>"
// then per source point "<d2 of the last iteration> <x> <y> <z>" of the aligned cloud (float32 bit patterns, hex).
#include "../csrc/icp.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace lmono;

static bool read_points(const char *path, std::vector<VmPoint> &pts)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); return false; }
    VmPoint p;
    while (std::fread(&p, sizeof p, 1, f) == 1) pts.push_back(p);
    std::fclose(f);
    return true;
}

static uint32_t bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }

// the largest off-diagonal the sweeps leave on the matrix icp_solve forms from s (the check the sweep count rests on)
static double offdiag(const IcpSums &s)
{
    double R[9], tau[3], A[16];
    icp_solve(s, R, tau, A);
    double m = 0.0;
    for (int i = 0; i < 4; i++) for (int k = 0; k < 4; k++) if (i != k && std::fabs(A[4 * i + k]) > m) m = std::fabs(A[4 * i + k]);
    return m;
}

int main(int argc, char **argv)
{
    if (argc != 9 && argc != 21) { std::fprintf(stderr, "usage: icp_test <target.bin> <source.bin> <max_corr> <max_iter> <eps> <mse_eps> <cell> <max_rings> [g0 .. g11]\n"); return 2; }
    const float D = std::strtof(argv[3], nullptr), h = std::strtof(argv[7], nullptr);
    const int max_iter = std::atoi(argv[4]), rings = std::atoi(argv[8]);
    const double eps = std::strtod(argv[5], nullptr), mse_eps = std::strtod(argv[6], nullptr);
    if (!icp_params_ok(D, max_iter, eps, mse_eps, h, rings)) {
        std::fprintf(stderr, "icp_test: 0 < max_corr <= 16, max_iter in 1 .. 65536, eps >= 0, mse_eps >= 0, cell > 0, max_rings in 1 .. 64, (max_rings - 0.25) cell >= max_corr\n");
        return 2;
    }
    double G[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    if (argc == 21) for (int k = 0; k < 12; k++) G[k] = std::strtod(argv[9 + k], nullptr);
    std::vector<VmPoint> tgt, src;
    if (!read_points(argv[1], tgt) || !read_points(argv[2], src)) return 1;
    const float inv = 1.0f / h, D2 = D * D;
    const size_t nt = tgt.size(), ns = src.size();

    // target: validity, origin, span
    std::vector<char> tok(nt, 0);
    uint32_t kmin[3] = { 0xffffffffu, 0xffffffffu, 0xffffffffu }, kmax[3] = { 0, 0, 0 };
    uint64_t key;
    int c[3];
    for (size_t i = 0; i < nt; i++) {
        tok[i] = sor_cell(tgt[i].x, tgt[i].y, tgt[i].z, inv, key, c);
        if (!tok[i]) continue;
        const uint32_t k[3] = { icp_ord(tgt[i].x), icp_ord(tgt[i].y), icp_ord(tgt[i].z) };
        for (int a = 0; a < 3; a++) { if (k[a] < kmin[a]) kmin[a] = k[a]; if (k[a] > kmax[a]) kmax[a] = k[a]; }
    }
    float o[3];
    for (int a = 0; a < 3; a++) o[a] = kmin[a] <= kmax[a] ? icp_origin(icp_unord(kmin[a]), icp_unord(kmax[a])) : 0.0f;
    int64_t t_rej = 0;
    for (size_t i = 0; i < nt; i++) {
        tok[i] = tok[i] && icp_in_span(tgt[i].x - o[0]) && icp_in_span(tgt[i].y - o[1]) && icp_in_span(tgt[i].z - o[2]);
        if (!tok[i]) t_rej++;
    }
    // source
    std::vector<float> u(3 * ns), d2(ns, INFINITY);
    std::vector<char> usable(ns, 0);
    int64_t s_bad = 0;
    for (size_t i = 0; i < ns; i++) {
        for (int a = 0; a < 3; a++) u[3 * i + a] = icp_guess_axis(G + 4 * a, src[i].x, src[i].y, src[i].z) - o[a];
        usable[i] = icp_in_span(u[3 * i]) && icp_in_span(u[3 * i + 1]) && icp_in_span(u[3 * i + 2]);
        if (!usable[i]) s_bad++;
    }
    IcpState st;
    icp_state_init(st);
    std::vector<int64_t> hist;
    double off = 0.0;
    while (ns > 0 && !st.done) {
        IcpSums sum;
        std::memset(&sum, 0, sizeof sum);
        for (size_t i = 0; i < ns; i++) {
            d2[i] = INFINITY;
            if (!usable[i]) continue;
            const float *ui = &u[3 * i];
            const float qx = icp_q_axis(st.R, st.tau[0], o[0], ui[0], ui[1], ui[2]), qy = icp_q_axis(st.R + 3, st.tau[1], o[1], ui[0], ui[1], ui[2]),
                        qz = icp_q_axis(st.R + 6, st.tau[2], o[2], ui[0], ui[1], ui[2]);
            if (!sor_cell(qx, qy, qz, inv, key, c)) continue;
            float best = INFINITY, bx = 0.0f, by = 0.0f, bz = 0.0f;
            for (size_t t = 0; t < nt; t++) {
                if (!tok[t]) continue;
                const float d = sor_d2(qx, qy, qz, tgt[t].x, tgt[t].y, tgt[t].z);
                if (icp_better(d, tgt[t].x, tgt[t].y, tgt[t].z, best, bx, by, bz)) { best = d; bx = tgt[t].x; by = tgt[t].y; bz = tgt[t].z; }
            }
            if (!(best <= D2)) continue;
            d2[i] = best;
            const float w[3] = { bx - o[0], by - o[1], bz - o[2] };
            IcpSums t;
            icp_terms(ui, w, best, t);
            long long *acc = (long long *)&sum;
            const long long *add = (const long long *)&t;
            for (int k = 0; k < kIcpWords; k++) acc[k] += add[k];
        }
        if (sum.N >= 3) { const double m = offdiag(sum); if (m > off) off = m; }
        icp_iterate(st, sum, max_iter, eps, mse_eps);
        hist.push_back(sum.N); hist.push_back(sum.E);
    }
    double T[12];
    icp_transform(st, o, G, T);
    std::printf("transform");
    for (int k = 0; k < 12; k++) { uint64_t b; std::memcpy(&b, &T[k], 8); std::printf(" %016" PRIx64, b); }
    std::printf("\nstats %zu %" PRId64 " %zu %" PRId64 " %d %d %lld %lld\n", ns, s_bad, nt, t_rej, st.k, st.status, st.last_n, st.last_e);
    std::printf("offdiag %g\n", off);
    std::printf("history %zu\n", hist.size() / 2);
    for (size_t k = 0; k < hist.size(); k += 2) std::printf("%" PRId64 " %" PRId64 "\n", hist[k], hist[k + 1]);
    for (size_t i = 0; i < ns; i++) {
        const float *ui = &u[3 * i];
        std::printf("%08x %08x %08x %08x\n", bits(d2[i]), bits(icp_q_axis(st.R, st.tau[0], o[0], ui[0], ui[1], ui[2])), bits(icp_q_axis(st.R + 3, st.tau[1], o[1], ui[0], ui[1], ui[2])),
                    bits(icp_q_axis(st.R + 6, st.tau[2], o[2], ui[0], ui[1], ui[2])));
    }
    return 0;
}
