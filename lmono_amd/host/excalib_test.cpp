// excalib_test.cpp -- the camera-LiDAR rotation calibration on the host, without a GPU: the arithmetic of
// ../csrc/excalib.hip compiled as plain C++ (-ffp-contract=off), in the kernel's order.
//   excalib_test <cases.bin>            results on stdout, every number as %.17g
//   excalib_test --time <cases.bin> K   the same cases K times, nothing printed but the steps per second
// cases: int32 n_sequences, then per sequence int32 count, int32 n_frames and per frame int32 kind (0: stages 1-3 alone, 1: the whole step,
// 2: stage 4 alone), int32 m, double pairs [m][4], double q_cam [4], double q_lidar [4] (x y z w; q_cam is read by kind 2 only).
// Every sequence starts from a fresh state.  Per frame one line:
//   REL <R 9> <stats 6>                                               kinds 0 and 1
//   CAL <rlc 9> <sv 4> <huber> <ok> <frame_count> <M 16>               kinds 1 and 2
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/excalib.hip"

template <typename T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static int run(const char *path, bool print, long *steps)
{
    FILE *in = fopen(path, "rb");
    if (!in) { fprintf(stderr, "excalib_test: cannot open %s\n", path); return 2; }
    int32_t n_seq = 0;
    if (!rd(in, &n_seq, 1) || n_seq < 0) { fprintf(stderr, "excalib_test: bad header\n"); fclose(in); return 1; }
    std::vector<double> pairs;
    for (int32_t s = 0; s < n_seq; s++) {
        int32_t count = 0, n_frames = 0;
        if (!rd(in, &count, 1) || !rd(in, &n_frames, 1) || count < 1 || n_frames < 0) { fprintf(stderr, "excalib_test: bad sequence %d\n", (int)s); fclose(in); return 1; }
        lmono::ExcState st;
        memset(&st, 0, sizeof(st));
        lmono::exc_identity(st.rlc);
        for (int32_t f = 0; f < n_frames; f++) {
            int32_t kind = 0, m = 0;
            double q_cam[4], q_lidar[4], R[9], rlc[9], sv[4], huber = 0.0;
            int stats[6];
            if (!rd(in, &kind, 1) || !rd(in, &m, 1) || kind < 0 || kind > 2 || m < 0 || m > lmono::kRejPts) { fprintf(stderr, "excalib_test: bad frame %d of sequence %d\n", (int)f, (int)s); fclose(in); return 1; }
            pairs.resize((size_t)m * 4);
            if (!rd(in, pairs.data(), pairs.size()) || !rd(in, q_cam, 4) || !rd(in, q_lidar, 4)) { fprintf(stderr, "excalib_test: short frame %d of sequence %d\n", (int)f, (int)s); fclose(in); return 1; }
            if (kind != 2) {
                lmono::exc_relative_host(m, pairs.data(), R, stats);
                if (print) {
                    printf("REL");
                    for (int e = 0; e < 9; e++) printf(" %.17g", R[e]);
                    for (int e = 0; e < 6; e++) printf(" %d", stats[e]);
                    printf("\n");
                }
                lmono::exc_m2q(R, q_cam);
            }
            if (kind != 0) {
                const bool ok = lmono::exc_calib(st, q_cam, q_lidar, count, rlc, sv, &huber);
                if (print) {
                    printf("CAL");
                    for (int e = 0; e < 9; e++) printf(" %.17g", rlc[e]);
                    for (int e = 0; e < 4; e++) printf(" %.17g", sv[e]);
                    printf(" %.17g %d %d", huber, ok ? 1 : 0, st.frame_count);
                    for (int e = 0; e < 16; e++) printf(" %.17g", st.M[e]);
                    printf("\n");
                }
            }
            (*steps)++;
        }
    }
    fclose(in);
    return 0;
}

int main(int argc, char **argv)
{
    long steps = 0;
    if (argc == 4 && std::string(argv[1]) == "--time") {
        const int K = atoi(argv[3]);
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < K; k++) if (int rc = run(argv[2], false, &steps)) return rc;
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("%ld steps in %.6f s: %.1f steps/s\n", steps, sec, sec > 0.0 ? (double)steps / sec : 0.0);
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: excalib_test [--time] <cases.bin> [K]\n"); return 2; }
    return run(argv[1], true, &steps);
}
