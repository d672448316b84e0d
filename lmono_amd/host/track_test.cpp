// lmono_amd/host/track_test.cpp -- synthetic frames -> FeatureTracker::trackImage (device tracker) -> FeatureManager::featureCheck.
// A textured plane (sinusoids + random rectangles) is cut out under a slow drift; every frame's feature frame has to be taken in by
// featureCheck in full: survivors extend their tracks, new ids open tracks, nothing else.  Prints one line per frame and "track_test ok".
//   track_test [frames [seed [reject]]]   seed 0: the default canvas; "reject": setRejectF(1.0, 0.5), plus one REJ line per frame
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "feature_tracker.hpp"

using namespace lmono_host;

static unsigned int g_seed = 12345u;
static double rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) / 16777216.0; }

int main(int argc, char **argv)
{
    const int n_frames = argc > 1 ? std::atoi(argv[1]) : 24;
    if (argc > 2 && std::atoi(argv[2]) != 0) g_seed = (unsigned int)std::atoi(argv[2]);
    const bool reject = argc > 3 && std::strcmp(argv[3], "reject") == 0;
    const int W = 320, H = 240, CW = 480, CH = 360;
    std::vector<double> canvas((size_t)CW * CH);
    for (int y = 0; y < CH; y++)
        for (int x = 0; x < CW; x++)
            canvas[(size_t)y * CW + x] = 128.0 + 25.0 * std::sin(0.21 * x + 0.13 * y) + 20.0 * std::sin(0.07 * x - 0.17 * y + 1.0) + 15.0 * std::sin(0.33 * y + 0.05 * x);
    for (int k = 0; k < 160; k++) {
        const int w = 6 + (int)(rnd() * 22), h = 6 + (int)(rnd() * 22), x0 = (int)(rnd() * (CW - w)), y0 = (int)(rnd() * (CH - h));
        const double d = -60.0 + 120.0 * rnd();
        for (int y = y0; y < y0 + h; y++) for (int x = x0; x < x0 + w; x++) canvas[(size_t)y * CW + x] += d;
    }
    try {
        HipContext hip(0);
        Params params;
        lmono_camera cam = { W, H, 300.0, 300.0, 160.0, 120.0, -0.1, 0.02, 0.0005, -0.0005, 5, 0, 0 };
        FeatureTracker tracker(hip, cam, 150, 15);
        if (reject) { tracker.setRejectF(1.0, 0.5); std::printf("rejectWithF on: F_THRESHOLD 1.0 F_DIS 0.5\n"); }
        FeatureManager fm;
        fm.params = &params; fm.hip = &hip;
        std::vector<uint8_t> bgr((size_t)W * H * 3);
        int frame_count = 0, keyframes = 0, last_id = -1;
        for (int f = 0; f < n_frames; f++) {
            const double tx = 60.0 + 1.7 * f, ty = 50.0 + 0.6 * f;
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    const double X = x + tx, Y = y + ty;
                    const int xi = (int)X, yi = (int)Y;
                    const double a = X - xi, b = Y - yi;
                    const double *p = &canvas[(size_t)yi * CW + xi];
                    double v = (1 - a) * (1 - b) * p[0] + a * (1 - b) * p[1] + (1 - a) * b * p[CW] + a * b * p[CW + 1];
                    v = v < 0 ? 0 : (v > 255 ? 255 : v);
                    const uint8_t g = (uint8_t)std::lrint(v);
                    uint8_t *o = &bgr[((size_t)y * W + x) * 3];
                    o[0] = o[1] = o[2] = g;
                }
            const FeatureTracker::FeatureFrame frame = tracker.trackImage(0.1 * f, bgr.data(), LMONO_TRACK_BGR8);
            const FeatureManager::Image image = FeatureTracker::toImage(frame);
            int survivors = 0, fresh = 0;
            for (const lmono_track_record &r : tracker.records) {
                if (r.track_cnt > 1) survivors++; else { fresh++; if (r.id <= last_id) { std::fprintf(stderr, "frame %d: id %d reused\n", f, r.id); return 1; } }
            }
            for (const lmono_track_record &r : tracker.records) if (r.id > last_id) last_id = r.id;
            if (image.size() != tracker.records.size() || (f == 0 && image.size() < 50)) { std::fprintf(stderr, "frame %d: %zu features\n", f, image.size()); return 1; }
            const bool keyframe = fm.featureCheck(frame_count, image, 0.0);
            int ending_here = 0;
            for (const FeaturePerId &t : fm.feature) if (t.endFrame() == frame_count) ending_here++;
            if (fm.last_track_num != survivors || fm.new_feature_num != fresh || ending_here != (int)image.size()) {
                std::fprintf(stderr, "frame %d: featureCheck took %d + %d (tracks ending here %d), the tracker gave %d + %d\n", f, fm.last_track_num, fm.new_feature_num, ending_here, survivors, fresh);
                return 1;
            }
            if (f > 0 && survivors < 50) { std::fprintf(stderr, "frame %d: only %d survivors\n", f, survivors); return 1; }
            keyframes += keyframe ? 1 : 0;
            if (reject) {
                const std::array<int32_t, 4> rs = tracker.rejectStats();
                std::printf("REJ %d valid %d best %d inliers %d kept %d\n", f, rs[0], rs[1], rs[2], rs[3]);
                if (f > 0 && (rs[0] <= 0 || rs[3] < 50)) { std::fprintf(stderr, "frame %d: rejectWithF kept %d\n", f, rs[3]); return 1; }
            }
            std::printf("TRK %d features %zu survivors %d new %d keyframe %d tracks %zu\n", f, image.size(), survivors, fresh, keyframe ? 1 : 0, fm.feature.size());
            if (frame_count == WINDOW_SIZE) fm.removeBack();       // slideWindow, MARGIN_OLD (Estimator.cc:700-771)
            else frame_count++;
        }
        std::printf("track_test ok: %d frames, %d keyframes\n", n_frames, keyframes);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "track_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
