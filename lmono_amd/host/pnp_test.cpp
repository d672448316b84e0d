// pnp_test.cpp -- the loop verification's PnP step on the host, without a GPU: the arithmetic of ../csrc/pnp.hip
// compiled as plain C++ (-ffp-contract=off), in the kernel's order.
//   pnp_test <problems.bin> <results.bin>
//   pnp_test --after <records.bin> <results.bin>      what follows the pose (KeyFrame.cc:341-350, :572-588, :658-682), the C ABI's host code
// problems: int32 n, then per problem int32 m, uint32 key, int32 n_hyp, uint32 seed, double threshold, double guess [7] (t, q x y z w),
// float points_3d [m][3], float points_2d_norm [m][2].  results: per problem uint8 status [m], int32 stats [4], double pose [7].
// records: int32 n, then per record double pose [7], vio [7], ex [7], old [7], angle_threshold, trans_threshold, current index.
// results: per record double PnP_T_old [3], PnP_q_old [4], loop_info [8], relative_euler [3], within (0 / 1), channel [15].
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../csrc/pnp.hip"

template <typename T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <typename T> static bool wr(FILE *f, const T *p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

static int after(const char *in_path, const char *out_path)
{
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) { fprintf(stderr, "pnp_test: cannot open the files\n"); return 2; }
    int32_t n = 0;
    if (!rd(in, &n, 1) || n < 0) { fprintf(stderr, "pnp_test: bad header\n"); return 1; }
    for (int32_t s = 0; s < n; s++) {
        double r[31], o[34];
        if (!rd(in, r, 31)) { fprintf(stderr, "pnp_test: short record %d\n", (int)s); return 1; }
        lmono::PnpLoop L;
        lmono::pnp_after(r, r + 7, r + 14, r[28], r[29], L);
        for (int e = 0; e < 3; e++) { o[e] = L.t_old[e]; o[15 + e] = L.rel_euler[e]; }
        for (int e = 0; e < 4; e++) o[3 + e] = L.q_old[e];
        lmono::pnp_loop_info(L, o + 7);
        o[18] = L.within ? 1.0 : 0.0;
        lmono::pnp_channel(r + 21, L, (int)r[30], o + 19);
        if (!wr(out, o, 34)) { fprintf(stderr, "pnp_test: write failed\n"); return 1; }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}

int main(int argc, char **argv)
{
    if (argc == 4 && std::string(argv[1]) == "--after") return after(argv[2], argv[3]);
    if (argc != 3) { fprintf(stderr, "usage: pnp_test [--after] <input.bin> <results.bin>\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "pnp_test: cannot open the files\n"); return 2; }
    int32_t n = 0;
    if (!rd(in, &n, 1) || n < 0) { fprintf(stderr, "pnp_test: bad header\n"); return 1; }
    for (int32_t s = 0; s < n; s++) {
        int32_t m = 0, n_hyp = 0;
        uint32_t key = 0, seed = 0;
        double thr = 0.0, guess[7], pose[7];
        if (!rd(in, &m, 1) || !rd(in, &key, 1) || !rd(in, &n_hyp, 1) || !rd(in, &seed, 1) || !rd(in, &thr, 1) || !rd(in, guess, 7) || m < 0 || m > lmono::kPnpPts ||
            n_hyp < 1 || n_hyp > lmono::kPnpMaxHyp) { fprintf(stderr, "pnp_test: bad problem %d\n", (int)s); return 1; }
        std::vector<float> p3((size_t)m * 3), p2((size_t)m * 2);
        std::vector<unsigned char> status((size_t)m);
        int32_t stats[4];
        if (!rd(in, p3.data(), p3.size()) || !rd(in, p2.data(), p2.size())) { fprintf(stderr, "pnp_test: short problem %d\n", (int)s); return 1; }
        lmono::pnp_ransac_host(m, p3.data(), p2.data(), guess, n_hyp, seed, key, thr * thr, status.data(), pose, stats);
        if (!wr(out, status.data(), status.size()) || !wr(out, stats, 4) || !wr(out, pose, 7)) { fprintf(stderr, "pnp_test: write failed\n"); return 1; }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
