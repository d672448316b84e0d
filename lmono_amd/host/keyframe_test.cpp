// lmono_amd/host/keyframe_test.cpp -- frames of an image sequence -> FeatureTracker::trackImage -> a KeyFrame from frame k and one from frame
// k + delta (window points: the tracker's points of that frame) -> findConnection up to the MIN_BRIEF_LOOP_NUM gate.  Prints the matches.
//   keyframe_test <frames.raw> <brief_pattern.yml> [k [delta]]
// frames.raw: a text line "<width> <height> <frames>" followed by frames * height * width grey bytes.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>
#include "feature_tracker.hpp"
#include "keyframe.hpp"

using namespace lmono_host;

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: keyframe_test <frames.raw> <brief_pattern.yml> [k [delta]]\n"); return 2; }
    const int k = argc > 3 ? std::atoi(argv[3]) : 2, delta = argc > 4 ? std::atoi(argv[4]) : 6;
    try {
        std::ifstream in(argv[1], std::ios::binary);
        int W = 0, H = 0, N = 0;
        in >> W >> H >> N;
        in.get();
        if (!in || W < 32 || H < 32 || W > 8192 || H > 8192 || k < 0 || delta < 1 || N < k + delta + 1) { std::fprintf(stderr, "keyframe_test: bad frames file or frame numbers\n"); return 2; }
        std::vector<uint8_t> frames((size_t)W * H * N);
        in.read((char *)frames.data(), (std::streamsize)frames.size());
        if ((size_t)in.gcount() != frames.size()) { std::fprintf(stderr, "keyframe_test: frames file is short\n"); return 2; }
        const lmono_brief_pattern pattern = loadBriefPattern(argv[2]);
        HipContext hip(0);
        lmono_camera cam = { W, H, 300.0, 300.0, 0.5 * W, 0.5 * H, -0.1, 0.02, 0.0005, -0.0005, 5, 0, 0 };
        FeatureTracker tracker(hip, cam, 150, 15);
        KeyFrameStore store(hip, cam, pattern, 8, 16384);
        std::vector<KeyFrame> kfs;
        kfs.reserve(2);
        for (int f = 0; f <= k + delta; f++) {
            const uint8_t *img = frames.data() + (size_t)f * W * H;
            tracker.trackImage(0.1 * f, img, LMONO_TRACK_GREY8);
            if (f != k && f != k + delta) continue;
            std::vector<Point3f> p3; std::vector<Point2f> uv, nm; std::vector<int> id;
            for (const lmono_track_record &r : tracker.records) {
                p3.push_back({ r.x_n, r.y_n, 1.f });            // no depth in this driver: the normalised ray stands in for point_3d
                uv.push_back({ r.u, r.v }); nm.push_back({ r.x_n, r.y_n }); id.push_back(r.id);
            }
            kfs.emplace_back(store, 0.1 * f, (int)kfs.size(), img, LMONO_TRACK_GREY8, p3, uv, nm, id, 0);
            std::printf("KF %d frame %d keypoints %zu window %zu\n", kfs.back().index, f, kfs.back().brief_keypoints.size(), kfs.back().window_brief_descriptors.size());
        }
        std::vector<Point2f> cur, old, cur_n, old_n; std::vector<Point3f> m3; std::vector<int> ids;
        const bool connected = kfs[1].findConnection(&kfs[0], cur, old, cur_n, old_n, m3, ids);
        for (size_t i = 0; i < ids.size(); i++)
            std::printf("MATCH %d cur %.9g %.9g old %.9g %.9g old_norm %.9g %.9g\n", ids[i], cur[i].x, cur[i].y, old[i].x, old[i].y, old_n[i].x, old_n[i].y);
        std::printf("keyframe_test ok: %zu of %zu window points matched, gate %d\n", ids.size(), kfs[1].point_2d_uv.size(), connected ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "keyframe_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
