// lmono_amd/host/feature_tracker.cpp -- see feature_tracker.hpp
#include "feature_tracker.hpp"

namespace lmono_host {

FeatureTracker::FeatureTracker(HipContext &hip, const lmono_camera &cam, int max_cnt, int min_dist)
    : hip_(hip), trk_(lmono_tracker_create(hip.get(), &cam, max_cnt, min_dist, 0))
{
    if (!trk_) throw std::runtime_error(std::string("lmono_tracker_create: ") + lmono_last_error(hip.get()));
}
FeatureTracker::~FeatureTracker() { lmono_tracker_destroy(trk_); }

void FeatureTracker::reset() { hip_.check(lmono_tracker_reset(hip_.get(), trk_), "lmono_tracker_reset"); }

void FeatureTracker::setRejectF(double f_threshold, double f_dis)
{
    const lmono_reject_f prm = { f_threshold, f_dis, 0.0, 0, 0u };
    hip_.check(lmono_tracker_set_reject_f(hip_.get(), trk_, &prm), "lmono_tracker_set_reject_f");
}
void FeatureTracker::clearRejectF() { hip_.check(lmono_tracker_set_reject_f(hip_.get(), trk_, nullptr), "lmono_tracker_set_reject_f"); }

std::array<int32_t, 4> FeatureTracker::rejectStats(std::array<double, 9> *F)
{
    std::array<int32_t, 4> stats;
    hip_.check(lmono_tracker_reject_stats(hip_.get(), trk_, stats.data(), F ? F->data() : nullptr), "lmono_tracker_reject_stats");
    return stats;
}

FeatureTracker::FeatureFrame FeatureTracker::trackImage(double cur_time, const uint8_t *image, int format)
{
    records.resize(LMONO_TRACK_MAX_POINTS);
    int n = 0;
    hip_.check(lmono_tracker_track(hip_.get(), trk_, cur_time, image, format, records.data(), (int)records.size(), &n), "lmono_tracker_track");
    records.resize((size_t)n);
    FeatureFrame frame;
    for (const lmono_track_record &r : records)
        frame[r.id].emplace_back(0, std::array<double, 6>{ r.x_n, r.y_n, r.u, r.v, r.vx, r.vy });
    return frame;
}

FeatureManager::Image FeatureTracker::toImage(const FeatureFrame &frame)
{
    FeatureManager::Image image;
    for (const auto &f : frame) {
        const std::array<double, 6> &v = f.second[0].second;
        image[f.first] = { v[0], v[1], v[2], v[3] };
    }
    return image;
}

} // namespace lmono_host
