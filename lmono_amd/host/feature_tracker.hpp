// lmono_amd/host/feature_tracker.hpp -- host-side mirror of FeatureTracker (mono_lidar_mapping/include/image_process/FeatureTracker.h)
// over the device tracker of the C ABI (lmono_tracker_*): trackImage(time, image) returns the reference's feature frame,
// whose first four values per feature are what Estimator::processImage takes (FeatureManager::Image).
#pragma once
#include <array>
#include <map>
#include <utility>
#include <vector>
#include "lmono_host.hpp"

namespace lmono_host {

class FeatureTracker {
public:
    // feature_id -> [(camera_id, x y u v vx vy)] (FeatureTracker.cc:372-397; the mono path has camera 0 only)
    typedef std::map<int, std::vector<std::pair<int, std::array<double, 6>>>> FeatureFrame;

    // max_cnt / min_dist: MAX_CNT (FeatureTracker.cc:21) / MIN_DIST of the config; use_rejectF: setRejectF below
    FeatureTracker(HipContext &hip, const lmono_camera &cam, int max_cnt = 150, int min_dist = 30);
    ~FeatureTracker();
    FeatureTracker(const FeatureTracker &) = delete;
    FeatureTracker &operator=(const FeatureTracker &) = delete;

    // image: [height][width] (format LMONO_TRACK_GREY8) or [height][width][3] BGR (LMONO_TRACK_BGR8) uint8
    FeatureFrame trackImage(double cur_time, const uint8_t *image, int format = LMONO_TRACK_BGR8);
    static FeatureManager::Image toImage(const FeatureFrame &frame);      // what processImage / featureCheck take
    void reset();
    // REJECT_F = 1 with F_THRESHOLD / F_DIS of the config (rejectWithF, FeatureTracker.cc:435-503; FOCAL_LENGTH 460), from the next frame on
    void setRejectF(double f_threshold, double f_dis);
    void clearRejectF();                                                  // REJECT_F = 0
    // last frame: valid hypotheses, best hypothesis, gate-1 inliers, kept after gate 2 (all -1: the step did not run)
    std::array<int32_t, 4> rejectStats(std::array<double, 9> *F = nullptr);

    std::vector<lmono_track_record> records;     // the frame as the device returned it: ids, cur_pts, cur_un_pts, pts_velocity, track_cnt in order
    lmono_tracker *get() const { return trk_; }

private:
    HipContext &hip_;
    lmono_tracker *trk_;
};

} // namespace lmono_host
