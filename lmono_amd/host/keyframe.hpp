// lmono_amd/host/keyframe.hpp -- host-side mirror of KeyFrame (mono_lidar_mapping/include/loop_detection/KeyFrame.h) over the device
// keyframe store of the C ABI (lmono_keyframes_*).  A KeyFrame keeps the reference's members on the host (they are read
// back once, when it is built) and its slot in the store; searchByBRIEFDes and findConnection run the search on the device.
// PnPRANSAC and findConnection to its end (KeyFrame.cc:296-351, :551-688) run on the device too (lmono_pnp_ransac, lmono_keyframes_verify).
// LoopDetector (below) mirrors LoopDetector.cc:26-260 over the store's BoW database (lmono_keyframes_detect_loop).
// Not mirrored: the USE_ORB branch, the thumbnail, DEBUG_IMAGE; the ROS message of :644-684 is the plain struct LoopMessage.
#pragma once
#include <array>
#include <list>
#include <string>
#include <vector>
#include "lmono_host.hpp"

namespace lmono_host {

struct Point2f { float x, y; };
struct Point3f { float x, y, z; };
typedef std::array<uint32_t, 8> BriefBits;           // BRIEF::bitset of 256 bits: bit i is bit i & 31 of word i >> 5

constexpr int MIN_BRIEF_LOOP_NUM = 25;               // kitti_config_00.yaml:48

// what :644-684 publishes on pub_matched_points_: one point (old normalised x, y, feature id) per verified match and the channel
// [old_T, old_Q (w x y z), correct_T, correct_Q (w x y z), index]
struct LoopMessage {
    double stamp = 0.0;
    std::vector<Point3f> points;
    double t_q_index[15] = { 0 };
};

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

    // KeyFrame.cc:296-351: solvePnPRansac of the matched pairs from the guess of :308-312 (origin_vio_tq, ex_tq) -> status (appended, one
    // byte per pair), PnP_T_old [3] and PnP_q_old [4] (x y z w).  The RANSAC is the definition of DESIGN.md 6g (lmono_pnp_ransac);
    // key selects its sample stream
    void PnPRANSAC(const std::vector<Point2f> &matched_2d_old_norm, const std::vector<Point3f> &matched_3d, std::vector<unsigned char> &status,
                   double *PnP_T_old, double *PnP_q_old, uint32_t key = 0);
    // KeyFrame.cc:354-691 in one device call (lmono_keyframes_verify): the match, PnPRANSAC, the three gates.  On true it has set has_loop,
    // loop_index, loop_info, point_loop_2d_norm, point_old_2d_norm, point_loop_id and published.  matched_brief / matched_pnp: the counts
    // compared with MIN_BRIEF_LOOP_NUM and MIN_PNP_LOOP_NUM
    bool findConnection(const KeyFrame *old_kf);

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
    // KeyFrame.cc:753-777; the mirror keeps one pose for vio_T_w_i / vio_R_w_i and T_w_i / R_w_i (updateVioPose sets the two alike)
    void getVioPose(double *tq) const { for (int e = 0; e < 7; e++) tq[e] = T_w_i_tq[e]; }
    void updateVioPose(const double *tq) { for (int e = 0; e < 7; e++) T_w_i_tq[e] = tq[e]; }

    // poses as t (x y z), q (x y z w): origin_vio_T / origin_vio_R, T_w_i / R_w_i, and the camera in the body (tlc, qlc); identity until set
    double origin_vio_tq[7] = { 0, 0, 0, 0, 0, 0, 1 }, T_w_i_tq[7] = { 0, 0, 0, 0, 0, 0, 1 }, ex_tq[7] = { 0, 0, 0, 0, 0, 0, 1 };
    lmono_pnp_params pnp_params = { 0.0, 0, 0u, 0, 0, 0.0, 0.0 };      // zeros: the defaults of kitti_loop_config_04.yaml
    double loop_info[8] = { 0 };                      // relative_t, relative_q (w x y z), relative_yaw (:638-640)
    std::vector<Point2f> point_loop_2d_norm, point_old_2d_norm;
    std::vector<int> point_loop_id;
    LoopMessage published;
    int matched_brief = 0, matched_pnp = 0;

private:
    KeyFrameStore &store_;
    void readBack();
};

// LoopDetector (include/loop_detection/Loop_Detector.h, src/loop_detection/LoopDetector.cc:26-150, :167-260) over one KeyFrameStore: the
// stored keyframes are the database (entry e is the keyframe in slot e, so db.add is the KeyFrame constructor's add), and db.query with
// the score rules is lmono_keyframes_detect_loop.  With keyframes built in order their index is their slot, as the reference assumes;
// detectLoop answers in keyframe indices either way.  Not mirrored: the drift members, the optimisation thread, the commented blocks,
// the files loop_odometry.txt / loop_recorder.txt, DEBUG_IMAGE.
class LoopDetector {
public:
    LoopDetector(KeyFrameStore &store, int loop_search_gap, double loop_search_time);      // LOOP_SEARCH_GAP, LOOP_SEARCH_TIME of the config
    ~LoopDetector();
    LoopDetector(const LoopDetector &) = delete;
    LoopDetector &operator=(const LoopDetector &) = delete;
    // :26-30: a file in the layout of VocabularyBinary.hpp; std::runtime_error with the library's reason for a malformed one
    void loadVocabulary(const std::string &voc_path);
    // :32-150: detectLoop, the LOOP_SEARCH_TIME gate, findConnection and the updateVioPose of :80-95 -> the loop's keyframe index or -1
    int addKeyFrame(KeyFrame *cur_kf, bool flag_detect_loop);
    // :167-260 -> the keyframe index of the loop candidate or -1; ret of db.query is left in ret_id (slots) / ret_score
    int detectLoop(KeyFrame *keyframe, int frame_index);
    KeyFrame *getKeyFrame(int index);                    // :152-165

    int LOOP_SEARCH_GAP;
    double LOOP_SEARCH_TIME;
    std::list<KeyFrame *> keyframelist;
    std::vector<int> ret_id;
    std::vector<double> ret_score;
private:
    KeyFrameStore &store_;
    lmono_brief_vocabulary *voc_ = nullptr;
};

} // namespace lmono_host
