// lmono_amd/host/keyframe_test.cpp -- frames of an image sequence -> FeatureTracker::trackImage -> a KeyFrame from frame k and one from frame
// k + delta (window points: the tracker's points of that frame) -> findConnection up to the MIN_BRIEF_LOOP_NUM gate.  Prints the matches.
//   keyframe_test <frames.raw> <brief_pattern.yml> [k [delta [verify]]]
// With `verify` the same lines are followed by findConnection to its end (PnPRANSAC, the gates, loop_info, the published message): the
// scene is taken as a fronto-parallel plane at 10 m in front of each camera, the current camera shifted by (0.3, 0.1, 0) m in the world.
//   keyframe_test <frames.raw> <brief_pattern.yml> detect <vocabulary.bin> [loop_search_gap [loop_search_time]]
// Every frame becomes a KeyFrame (window points: the tracker's points) and goes through LoopDetector::addKeyFrame(kf, true) with a
// vocabulary file in the layout of VocabularyBinary.hpp; one line per keyframe: its loop index and the results of db.query.
// frames.raw: a text line "<width> <height> <frames>" followed by frames * height * width grey bytes.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "feature_tracker.hpp"
#include "keyframe.hpp"

using namespace lmono_host;

static int detect(int argc, char **argv)
{
    if (argc < 5) { std::fprintf(stderr, "usage: keyframe_test <frames.raw> <brief_pattern.yml> detect <vocabulary.bin> [loop_search_gap [loop_search_time]]\n"); return 2; }
    const int gap = argc > 5 ? std::atoi(argv[5]) : 100;
    const double search_time = argc > 6 ? std::atof(argv[6]) : 1e9;
    try {
        std::ifstream in(argv[1], std::ios::binary);
        int W = 0, H = 0, N = 0;
        in >> W >> H >> N;
        in.get();
        if (!in || W < 32 || H < 32 || W > 8192 || H > 8192 || N < 1 || N > 4096) { std::fprintf(stderr, "keyframe_test: bad frames file\n"); return 2; }
        std::vector<uint8_t> frames((size_t)W * H * N);
        in.read((char *)frames.data(), (std::streamsize)frames.size());
        if ((size_t)in.gcount() != frames.size()) { std::fprintf(stderr, "keyframe_test: frames file is short\n"); return 2; }
        const lmono_brief_pattern pattern = loadBriefPattern(argv[2]);
        HipContext hip(0);
        lmono_camera cam = { W, H, 300.0, 300.0, 0.5 * W, 0.5 * H, -0.1, 0.02, 0.0005, -0.0005, 5, 0, 0 };
        FeatureTracker tracker(hip, cam, 150, 15);
        KeyFrameStore store(hip, cam, pattern, N, 16384);
        LoopDetector detector(store, gap, search_time);
        detector.loadVocabulary(argv[4]);
        std::vector<KeyFrame> kfs;
        kfs.reserve((size_t)N);
        for (int f = 0; f < N; f++) {
            const uint8_t *img = frames.data() + (size_t)f * W * H;
            tracker.trackImage(0.1 * f, img, LMONO_TRACK_GREY8);
            std::vector<Point3f> p3; std::vector<Point2f> uv, nm; std::vector<int> id;
            for (const lmono_track_record &r : tracker.records) {
                p3.push_back({ r.x_n, r.y_n, 1.f }); uv.push_back({ r.u, r.v }); nm.push_back({ r.x_n, r.y_n }); id.push_back(r.id);
            }
            kfs.emplace_back(store, 0.1 * f, f, img, LMONO_TRACK_GREY8, p3, uv, nm, id, 0);
            const int loop = detector.addKeyFrame(&kfs.back(), true);
            std::printf("DETECT %d keypoints %zu loop %d results %zu", f, kfs.back().brief_keypoints.size(), loop, detector.ret_id.size());
            for (size_t i = 0; i < detector.ret_id.size(); i++) std::printf(" %d:%.17g", detector.ret_id[i], detector.ret_score[i]);
            std::printf("\n");
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "keyframe_test: %s\n", e.what());
        return 1;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: keyframe_test <frames.raw> <brief_pattern.yml> [k [delta [verify]]] | detect <vocabulary.bin> [gap [time]]\n"); return 2; }
    if (argc > 3 && std::string(argv[3]) == "detect") return detect(argc, argv);
    const int k = argc > 3 ? std::atoi(argv[3]) : 2, delta = argc > 4 ? std::atoi(argv[4]) : 6;
    const bool verify = argc > 5 && std::string(argv[5]) == "verify";
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
                // no depth in this driver: the normalised ray stands in for point_3d; with `verify` the ray at 10 m, moved into the world by the camera's shift
                if (verify) p3.push_back({ r.x_n * 10.f + (f == k ? 0.f : 0.3f), r.y_n * 10.f + (f == k ? 0.f : 0.1f), 10.f });
                else p3.push_back({ r.x_n, r.y_n, 1.f });
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
        if (verify) {
            KeyFrame &cur_kf = kfs[1];
            cur_kf.origin_vio_tq[0] = 0.3; cur_kf.origin_vio_tq[1] = 0.1;
            cur_kf.T_w_i_tq[0] = 0.3; cur_kf.T_w_i_tq[1] = 0.1;
            // PnPRANSAC on the reduced vectors of the seven-argument findConnection above, as :560 calls it
            std::vector<unsigned char> pnp_status;
            double T_old[3], q_old[4];
            cur_kf.PnPRANSAC(old_n, m3, pnp_status, T_old, q_old);
            int pnp_in = 0;
            for (unsigned char b : pnp_status) pnp_in += b;
            std::printf("PNPRANSAC pairs %zu inliers %d T_old %.17g %.17g %.17g q_old %.17g %.17g %.17g %.17g\n", pnp_status.size(), pnp_in, T_old[0], T_old[1], T_old[2],
                        q_old[0], q_old[1], q_old[2], q_old[3]);
            const bool loop = cur_kf.findConnection(&kfs[0]);
            std::printf("VERIFY brief %d pnp %d has_loop %d loop_index %d\n", cur_kf.matched_brief, cur_kf.matched_pnp, loop ? 1 : 0, cur_kf.loop_index);
            if (loop) {
                std::printf("LOOP_INFO");
                for (int e = 0; e < 8; e++) std::printf(" %.9g", cur_kf.loop_info[e]);
                std::printf("\nCHANNEL");
                for (int e = 0; e < 15; e++) std::printf(" %.9g", cur_kf.published.t_q_index[e]);
                std::printf("\n");
                for (size_t i = 0; i < cur_kf.point_loop_id.size(); i++)
                    std::printf("LOOP_POINT %d cur_norm %.9g %.9g old_norm %.9g %.9g published %.9g %.9g %.9g\n", cur_kf.point_loop_id[i], cur_kf.point_loop_2d_norm[i].x,
                                cur_kf.point_loop_2d_norm[i].y, cur_kf.point_old_2d_norm[i].x, cur_kf.point_old_2d_norm[i].y, cur_kf.published.points[i].x,
                                cur_kf.published.points[i].y, cur_kf.published.points[i].z);
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "keyframe_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
