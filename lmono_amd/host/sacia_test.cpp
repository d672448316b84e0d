// lmono_amd/host/sacia_test.cpp -- the sample-consensus initial alignment on the host: the whole definition by brute force with
// csrc/sacia.hpp, the text the kernels run; no GPU library.
//   sacia_test <src_kp.bin> <src_desc.bin> <src_flag.bin> <tgt_kp.bin> <tgt_desc.bin> <tgt_flag.bin> <min_sample_dist> <max_corr> <k_corr> <n_hyp> <seed>
// kp: [m][3] float32, desc: [m][33] float32, flag: [m] uint32.  Prints
//   stats <ok> <winning h> <its error word> <its inliers> <void hypotheses> <usable source keypoints> <usable target keypoints> <n_hyp>
//   T <12 doubles as bit patterns, hex> | T none
// then per hypothesis its error word (all ones: void) and its inliers.  Exit status 3: refused as LMONO_EINVAL (fewer than 3 usable keypoints on
// a side, or one out of span).
#include "../csrc/sacia.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace lmono;

template <typename T> static bool read_all(const char *path, std::vector<T> &out)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); return false; }
    T v;
    while (std::fread(&v, sizeof v, 1, f) == 1) out.push_back(v);
    std::fclose(f);
    return true;
}

struct Side { std::vector<float> kp, desc; std::vector<uint32_t> flag; std::vector<float> pos, d, c; };   // pos, d: the usable ones; c: centred

static bool load(char **argv, Side &s)
{
    if (!read_all(argv[0], s.kp) || !read_all(argv[1], s.desc) || !read_all(argv[2], s.flag)) return false;
    const size_t m = s.flag.size();
    if (s.kp.size() != 3 * m || s.desc.size() != (size_t)kFpfhDim * m || m > (size_t)kFpfhMaxKeypoints) { std::fprintf(stderr, "sacia_test: sizes do not agree\n"); return false; }
    for (size_t k = 0; k < m; k++)
        if (s.flag[k] == 1u) {
            s.pos.insert(s.pos.end(), s.kp.begin() + 3 * k, s.kp.begin() + 3 * k + 3);
            s.d.insert(s.d.end(), s.desc.begin() + kFpfhDim * k, s.desc.begin() + kFpfhDim * (k + 1));
        }
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 12) { std::fprintf(stderr, "usage: sacia_test <src kp desc flag> <tgt kp desc flag> <min_sample_dist> <max_corr> <k_corr> <n_hyp> <seed>\n"); return 2; }
    const float msd = std::strtof(argv[7], nullptr), mc = std::strtof(argv[8], nullptr);
    const int k_corr = std::atoi(argv[9]), n_hyp = std::atoi(argv[10]);
    const uint32_t seed = (uint32_t)std::strtoul(argv[11], nullptr, 10);
    if (!sacia_params_ok(msd, mc, k_corr, n_hyp)) { std::fprintf(stderr, "sacia_test: 0 <= min_sample_dist <= 4096, 0 < max_corr <= 16, k_corr in 1 .. 32, n_hyp in 1 .. 65536\n"); return 2; }
    Side S, T;
    if (!load(argv + 1, S) || !load(argv + 4, T)) return 1;
    const int ns = (int)(S.pos.size() / 3), nt = (int)(T.pos.size() / 3);
    if (ns < 3 || nt < 3) return 3;
    bool span = true;
    S.c.resize(S.pos.size()); T.c.resize(T.pos.size());
    for (size_t e = 0; e < S.pos.size(); e++) { S.c[e] = S.pos[e] - S.pos[e % 3]; span = span && icp_in_span(S.c[e]); }
    for (size_t e = 0; e < T.pos.size(); e++) { T.c[e] = T.pos[e] - T.pos[e % 3]; span = span && icp_in_span(T.c[e]); }
    if (!span) return 3;
    const int K = k_corr < nt ? k_corr : nt;
    const float msd2 = msd * msd, mc2 = mc * mc;

    // candidates: K rounds of the least (D, j) after the one taken before
    std::vector<int> cand((size_t)ns * K);
    std::vector<float> D((size_t)nt);
    for (int i = 0; i < ns; i++) {
        for (int j = 0; j < nt; j++) D[j] = sacia_desc_d2(&S.d[(size_t)i * kFpfhDim], &T.d[(size_t)j * kFpfhDim]);
        float pd = -1.0f;
        int pj = -1;
        for (int k = 0; k < K; k++) {
            float bd = INFINITY;
            int bj = nt;
            for (int j = 0; j < nt; j++)
                if (sacia_before(pd, pj, D[j], j) && sacia_before(D[j], j, bd, bj)) { bd = D[j]; bj = j; }
            cand[(size_t)i * K + k] = bj < nt ? bj : nt - 1;
            pd = bd; pj = bj;
        }
    }
    std::vector<unsigned long long> err((size_t)n_hyp, kSaciaVoid);
    std::vector<unsigned> inl((size_t)n_hyp, 0u);
    unsigned long long be = kSaciaVoid;
    int bh = -1, voids = 0;
    double bT[12] = { 0 };
    for (int h = 0; h < n_hyp; h++) {
        double R[9], tau[3];
        if (!sacia_fit(pnp_key(seed, kSaciaKey, (uint32_t)h), ns, S.c.data(), T.c.data(), cand.data(), K, msd2, R, tau)) { voids++; continue; }
        unsigned long long e = 0;
        for (int i = 0; i < ns; i++) {
            const float *u = &S.c[3 * (size_t)i];
            const float qx = icp_q_axis(R, tau[0], T.pos[0], u[0], u[1], u[2]), qy = icp_q_axis(R + 3, tau[1], T.pos[1], u[0], u[1], u[2]), qz = icp_q_axis(R + 6, tau[2], T.pos[2], u[0], u[1], u[2]);
            float best = INFINITY;
            for (int j = 0; j < nt; j++) {
                const float d2 = sor_d2(qx, qy, qz, T.pos[3 * (size_t)j], T.pos[3 * (size_t)j + 1], T.pos[3 * (size_t)j + 2]);
                if (d2 < best) best = d2;
            }
            e += sacia_term(best, mc2);
            inl[h] += best <= mc2 ? 1u : 0u;
        }
        err[h] = e;
        if (bh < 0 || e < be) { be = e; bh = h; sacia_transform(R, tau, S.pos.data(), T.pos.data(), bT); }
    }
    std::printf("stats %d %d %llu %u %d %d %d %d\n", bh >= 0 ? 1 : 0, bh, bh >= 0 ? be : 0ull, bh >= 0 ? inl[bh] : 0u, voids, ns, nt, n_hyp);
    if (bh >= 0) {
        std::printf("T");
        for (int e = 0; e < 12; e++) { uint64_t b; std::memcpy(&b, &bT[e], 8); std::printf(" %016" PRIx64, b); }
        std::printf("\n");
    } else std::printf("T none\n");
    for (int h = 0; h < n_hyp; h++) std::printf("%llu %u\n", err[h], inl[h]);
    return 0;
}
