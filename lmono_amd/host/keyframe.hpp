// lmono_amd/host/keyframe.hpp -- host-side mirror of KeyFrame (mono_lidar_mapping/include/loop_detection/KeyFrame.h) over the device
// keyframe store of the C ABI (lmono_keyframes_*).  A KeyFrame keeps the reference's members on the host (they are read
// back once, when it is built) and its slot in the store; searchByBRIEFDes and findConnection run the search on the device.
// Not mirrored: the DBoW2 database, PnPRANSAC and what follows it (KeyFrame.cc:551-688), the USE_ORB branch, the thumbnail, DEBUG_IMAGE.
#pragma once
#include <array>
#include <string>
#include <vector>
#include "lmono_host.hpp"

namespace lmono_host {

struct Point2f { float x, y; };
struct Point3f { float x, y, z; };
typedef std::array<uint32_t, 8> BriefBits;           // BRIEF::bitset of 256 bits: bit i is bit i & 31 of word i >> 5

constexpr int MIN_BRIEF_LOOP_NUM = 25;               // kitti_config_00.yaml:48

// BRIEF_PATTERN_FILE: an OpenCV-YAML file in the list layout of the reference's brief_pattern.yml (`x1:` followed by one `- <integer>` line
// per entry, likewise y1, x2, y2).  Throws std::runtime_error unless it finds exactly 256 entries per key, each in -63..63.
lmono_brief_pattern loadBriefPattern(const std::string &path);

// the device store every KeyFrame of one sequence lives in
class KeyFrameStore {
public:
    KeyFrameStore(HipContext &hip, const lmono_camera &cam, const lmono_brief_pattern &pattern, int max_keyframes = 1024, int max_keypoints = 8192, int fast_threshold = 0);
    ~KeyFrameStore();
    KeyFrameStore(const KeyFrameStore &) = delete;
    KeyFrameStore &operator=(const KeyFrameStore &) = delete;
    lmono_keyframes *get() const { return kfs_; }
    HipContext &hip() const { return hip_; }
private:
    HipContext &hip_;
    lmono_keyframes *kfs_;
};

class KeyFrame {
public:
    // create keyframe online (KeyFrame.cc:14-93): computeWindowBRIEFPoint + computeBRIEFPoint on the device
    KeyFrame(KeyFrameStore &store, double _time_stamp, int _index, const uint8_t *_image, int format, const std::vector<Point3f> &_point_3d,
             const std::vector<Point2f> &_point_2d_uv, const std::vector<Point2f> &_point_2d_norm, const std::vector<int> &_point_id, int _sequence);
    // load previous keyframe (KeyFrame.cc:96-133)
    KeyFrame(KeyFrameStore &store, double _time_stamp, int _index, int _loop_index, const std::vector<Point2f> &_keypoints,
             const std::vector<Point2f> &_keypoints_norm, const std::vector<BriefBits> &_brief_descriptors);

    // KeyFrame.cc:248-267 against old's brief_descriptors / brief_keypoints / brief_keypoints_norm
    void searchByBRIEFDes(std::vector<Point2f> &matched_2d_old, std::vector<Point2f> &matched_2d_old_norm, std::vector<unsigned char> &status, const KeyFrame *old_kf);
    // KeyFrame.cc:455-462 and the gate of :557: the matched_* vectors reduced by status, as PnPRANSAC would receive them; true when more
    // than MIN_BRIEF_LOOP_NUM points matched
    bool findConnection(const KeyFrame *old_kf, std::vector<Point2f> &matched_2d_cur, std::vector<Point2f> &matched_2d_old, std::vector<Point2f> &matched_2d_cur_norm,
                        std::vector<Point2f> &matched_2d_old_norm, std::vector<Point3f> &matched_3d, std::vector<int> &matched_id);

    double time_stamp;
    int index;
    int store_index;                                  // slot in the device store
    std::vector<Point3f> point_3d;
    std::vector<Point2f> point_2d_uv, point_2d_norm;
    std::vector<int> point_id;
    std::vector<Point2f> brief_keypoints, brief_keypoints_norm;
    std::vector<BriefBits> brief_descriptors, window_brief_descriptors;
    int sequence;
    bool has_loop;
    int loop_index;

private:
    KeyFrameStore &store_;
    void readBack();
};

} // namespace lmono_host
