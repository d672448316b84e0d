// lmono_amd/host/batch_api_test.cpp -- the contract of EstimatorBatch's stream interface, on window-filling frames only (no solve: it runs over any
// implementation of the C ABI, the CPU baseline of the frame loop included): absent streams, addStream / resetStream, the capacity, and the refusal of
// ESTIMATE_LASER == 2 where the C ABI has no calibration.  Prints "ok <check>" per check and "batch_api_test: all ok"; the first failure ends it with status 1.
// The last check expects a C ABI without lmono_excalib_* (the CPU baseline); tests/test_estimator_async_cpu.py builds and runs it that way.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "lmono_host.hpp"

using namespace lmono_host;

static void ok(bool cond, const char *what)
{
    if (!cond) { std::fprintf(stderr, "batch_api_test: FAILED %s\n", what); std::exit(1); }
    std::printf("ok %s\n", what);
}
template <typename E, typename F> static bool throws(F f)
{
    try { f(); } catch (const E &) { return true; } catch (...) { return false; }
    return false;
}

// frame k of a toy stream: eight tracked points that drift with k, the LiDAR 0.2 m further along x
static FeatureManager::Image image_of(int k, int stream)
{
    FeatureManager::Image im;
    for (int i = 0; i < 8; i++) im[i] = { 0.05 * i - 0.2 + 0.002 * k + 0.001 * stream, 0.03 * i - 0.1, 400.0 + 20 * i + k, 200.0 + 10 * i };
    return im;
}
static void pose_of(int k, double T[16])
{
    std::memset(T, 0, 16 * sizeof(double));
    T[0] = T[5] = T[10] = T[15] = 1.0; T[3] = 0.2 * k;
}

int main()
{
    try {
        HipContext hip(0);
        Params p;
        EstimatorBatch eb(hip, p, 2, 2, 3);
        ok(eb.size() == 2 && eb.capacity() == 3, "a batch of 2 streams with room for 3");
        std::vector<int> hook_calls(3, 0);
        eb.setFrameHook([&hook_calls](int s, const Estimator &) { hook_calls[(size_t)s]++; });

        double headers[3] = { 0, 0, 0 }, L0[3][16];
        FeatureManager::Image im[3];
        const FeatureManager::Image *img[3] = { nullptr, nullptr, nullptr };
        bool kf[3] = { true, true, true };

        // an all-absent call changes nothing, and Finish after it is a no-op too
        eb.processImageBegin(headers, img, L0, kf);
        eb.processImageFinish();
        ok(eb.stream(0).frame_count == 0 && eb.stream(1).frame_count == 0 && eb.stream(0).feature_manager.feature.empty(), "an all-absent call is a no-op");
        ok(!kf[0] && !kf[1] && hook_calls[0] == 0 && hook_calls[1] == 0, "an all-absent call reports no keyframe and calls no hook");
        ok(!throws<std::logic_error>([&] { eb.addStream(); }) && eb.size() == 3, "addStream after an all-absent call (no frame is open)");

        // stream 1 absent: stream 0 and 2 advance, stream 1 stays as it is; headers / poses of the absent stream are not read (they are NaN here)
        for (int k = 0; k < 3; k++) {
            for (int s = 0; s < 3; s++) { im[s] = image_of(k, s); pose_of(k, L0[s]); headers[s] = 0.1 * k; }
            headers[1] = std::nan(""); for (double &v : L0[1]) v = std::nan("");
            img[0] = &im[0]; img[1] = nullptr; img[2] = &im[2];
            kf[1] = true;
            eb.processImage(headers, img, L0, kf);
            ok(!kf[1], "keyframe[s] is false for an absent stream");
        }
        ok(eb.stream(0).frame_count == 3 && eb.stream(2).frame_count == 3 && eb.stream(1).frame_count == 0 && eb.stream(1).feature_manager.feature.empty(),
           "an absent stream does not change");
        ok(hook_calls[0] == 3 && hook_calls[2] == 3 && hook_calls[1] == 0, "the hook is not called for an absent stream");
        ok(eb.stream(1).last_laser_t.v[0] == 0.0 && eb.stream(0).prev_laser_pose[3] == 0.2 * 2, "prev_laser_pose follows the frames a stream was given");

        // between Begin and Finish the set of streams is fixed
        img[1] = &im[1]; pose_of(3, L0[1]); headers[1] = 0.3;
        eb.processImageBegin(headers, img, L0, kf);
        ok(throws<std::logic_error>([&] { eb.addStream(); }), "addStream between Begin and Finish throws std::logic_error");
        ok(throws<std::logic_error>([&] { eb.resetStream(0); }), "resetStream between Begin and Finish throws std::logic_error");
        eb.processImageFinish();
        ok(eb.stream(0).frame_count == 4 && eb.stream(1).frame_count == 1, "the frame between them ran");

        // the capacity
        ok(throws<std::length_error>([&] { eb.addStream(); }) && eb.size() == 3, "addStream beyond the capacity throws");

        // resetStream: a fresh Estimator in the same slot
        Estimator &fresh = eb.resetStream(0);
        ok(&fresh == &eb.stream(0) && fresh.frame_count == 0 && fresh.stage_flag == Estimator::NOT_INITED && fresh.feature_manager.feature.empty() && fresh.TLC[0] == 1.0,
           "resetStream returns a fresh NOT_INITED Estimator");
        ok(eb.stream(2).frame_count == 4, "resetStream leaves the other streams alone");
        img[1] = nullptr; img[2] = nullptr;
        eb.processImage(headers, img, L0, kf);
        ok(eb.stream(0).frame_count == 1 && eb.stream(2).frame_count == 4, "the restarted stream runs alone");

        // ESTIMATE_LASER == 2: the first frame that calibrates (frame_count > 0) needs lmono_excalib_*
        Params p2; p2.ESTIMATE_LASER = 2;
        EstimatorBatch cal(hip, p2, 2);
        const FeatureManager::Image *img2[2] = { &im[0], &im[1] };
        cal.processImage(headers, img2, L0, kf);                          // frame 0 forms no pair
        bool refused = false; std::string msg;
        try { cal.processImage(headers, img2, L0, kf); } catch (const std::runtime_error &e) { refused = true; msg = e.what(); }
        std::string single_msg;
        {
            Estimator one(hip, p2);
            one.processImage(headers[0], im[0], L0[0]);
            try { one.processImage(headers[0], im[0], L0[0]); } catch (const std::runtime_error &e) { single_msg = e.what(); }
        }
        ok(refused && !single_msg.empty() && msg == single_msg, "ESTIMATE_LASER == 2 is refused on this link with the single Estimator's message");
        ok(!throws<std::logic_error>([&] { cal.resetStream(1); }), "the refused call leaves no frame open");
        std::printf("batch_api_test: all ok\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "batch_api_test: %s\n", e.what());
        return 1;
    }
}
