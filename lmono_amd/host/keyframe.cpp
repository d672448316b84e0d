// lmono_amd/host/keyframe.cpp -- see keyframe.hpp
#include "keyframe.hpp"
#include <cstdlib>
#include <fstream>
#include <map>

namespace lmono_host {

lmono_brief_pattern loadBriefPattern(const std::string &path)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error("loadBriefPattern: cannot open " + path);
    std::map<std::string, std::vector<long>> got;
    std::string line, cur;
    int no = 0;
    while (std::getline(in, line)) {
        no++;
        if (!line.empty() && line[0] == '%') continue;
        line = line.substr(0, line.find('#'));
        const size_t a = line.find_first_not_of(" \t\r"), b = line.find_last_not_of(" \t\r");
        if (a == std::string::npos) continue;
        line = line.substr(a, b - a + 1);
        if (line == "---") continue;
        const std::string where = path + ":" + std::to_string(no);
        if (line.back() == ':') {
            cur = line.substr(0, line.find_last_not_of(" \t:") + 1);
            if (cur != "x1" && cur != "y1" && cur != "x2" && cur != "y2") throw std::runtime_error(where + ": not a key of a BRIEF pattern: " + line);
            if (got.count(cur)) throw std::runtime_error(where + ": key " + cur + " appears twice");
            got[cur];
        } else if (line[0] == '-' && !cur.empty()) {
            const std::string num = line.substr(line.find_first_not_of(" \t", 1) == std::string::npos ? line.size() : line.find_first_not_of(" \t", 1));
            char *end = nullptr;
            const long v = std::strtol(num.c_str(), &end, 10);
            if (num.empty() || *end != '\0') throw std::runtime_error(where + ": not an integer entry: " + line);
            got[cur].push_back(v);
        } else throw std::runtime_error(where + ": not a line of a BRIEF pattern list: " + line);
    }
    lmono_brief_pattern p;
    const char *keys[4] = { "x1", "y1", "x2", "y2" };
    int8_t *dst[4] = { p.x1, p.y1, p.x2, p.y2 };
    for (int k = 0; k < 4; k++) {
        const std::vector<long> &v = got[keys[k]];
        if (v.size() != 256) throw std::runtime_error(path + ": key " + keys[k] + " has " + std::to_string(v.size()) + " entries, a BRIEF pattern needs exactly 256");
        for (int i = 0; i < 256; i++) {
            if (v[(size_t)i] < -63 || v[(size_t)i] > 63) throw std::runtime_error(path + ": key " + keys[k] + ": an offset lies outside -63..63");
            dst[k][i] = (int8_t)v[(size_t)i];
        }
    }
    return p;
}

KeyFrameStore::KeyFrameStore(HipContext &hip, const lmono_camera &cam, const lmono_brief_pattern &pattern, int max_keyframes, int max_keypoints, int fast_threshold)
    : hip_(hip), kfs_(lmono_keyframes_create(hip.get(), &cam, &pattern, max_keyframes, max_keypoints, fast_threshold))
{
    if (!kfs_) throw std::runtime_error(std::string("lmono_keyframes_create: ") + lmono_last_error(hip.get()));
}
KeyFrameStore::~KeyFrameStore() { lmono_keyframes_destroy(kfs_); }

KeyFrame::KeyFrame(KeyFrameStore &store, double _time_stamp, int _index, const uint8_t *_image, int format, const std::vector<Point3f> &_point_3d,
                   const std::vector<Point2f> &_point_2d_uv, const std::vector<Point2f> &_point_2d_norm, const std::vector<int> &_point_id, int _sequence)
    : time_stamp(_time_stamp), index(_index), store_index(-1), point_3d(_point_3d), point_2d_uv(_point_2d_uv), point_2d_norm(_point_2d_norm), point_id(_point_id),
      sequence(_sequence), has_loop(false), loop_index(-1), store_(store)
{
    int n_kp = 0;
    store.hip().check(lmono_keyframes_add(store.hip().get(), store.get(), _image, format, (int)point_2d_uv.size(), point_2d_uv.empty() ? nullptr : &point_2d_uv[0].x,
                                          &store_index, &n_kp), "lmono_keyframes_add");
    readBack();
}

KeyFrame::KeyFrame(KeyFrameStore &store, double _time_stamp, int _index, int _loop_index, const std::vector<Point2f> &_keypoints,
                   const std::vector<Point2f> &_keypoints_norm, const std::vector<BriefBits> &_brief_descriptors)
    : time_stamp(_time_stamp), index(_index), store_index(-1), brief_keypoints(_keypoints), brief_keypoints_norm(_keypoints_norm), brief_descriptors(_brief_descriptors),
      sequence(0), has_loop(_loop_index != -1), loop_index(_loop_index), store_(store)
{
    if (_keypoints.size() != _keypoints_norm.size() || _keypoints.size() != _brief_descriptors.size()) throw std::runtime_error("KeyFrame: keypoints, keypoints_norm and descriptors differ in length");
    const bool none = _keypoints.empty();
    store.hip().check(lmono_keyframes_load(store.hip().get(), store.get(), (int)_keypoints.size(), none ? nullptr : &brief_keypoints[0].x, none ? nullptr : &brief_keypoints_norm[0].x,
                                           none ? nullptr : brief_descriptors[0].data(), 0, nullptr, nullptr, &store_index), "lmono_keyframes_load");
}

void KeyFrame::readBack()
{
    lmono_ctx *c = store_.hip().get();
    int n_kp = 0, n_win = 0;
    store_.hip().check(lmono_keyframes_get(c, store_.get(), store_index, &n_kp, nullptr, nullptr, nullptr, &n_win, nullptr, nullptr), "lmono_keyframes_get");
    brief_keypoints.resize((size_t)n_kp); brief_keypoints_norm.resize((size_t)n_kp); brief_descriptors.resize((size_t)n_kp); window_brief_descriptors.resize((size_t)n_win);
    store_.hip().check(lmono_keyframes_get(c, store_.get(), store_index, nullptr, n_kp ? &brief_keypoints[0].x : nullptr, n_kp ? &brief_keypoints_norm[0].x : nullptr,
                                           n_kp ? brief_descriptors[0].data() : nullptr, nullptr, nullptr, n_win ? window_brief_descriptors[0].data() : nullptr), "lmono_keyframes_get");
}

void KeyFrame::searchByBRIEFDes(std::vector<Point2f> &matched_2d_old, std::vector<Point2f> &matched_2d_old_norm, std::vector<unsigned char> &status, const KeyFrame *old_kf)
{
    const size_t n = window_brief_descriptors.size();
    const size_t at = status.size();                     // the reference appends (push_back)
    status.resize(at + n); matched_2d_old.resize(matched_2d_old.size() + n); matched_2d_old_norm.resize(matched_2d_old_norm.size() + n);
    if (n == 0) return;
    const int32_t old_index = old_kf->store_index;
    store_.hip().check(lmono_keyframes_match(store_.hip().get(), store_.get(), store_index, 1, &old_index, &status[at], nullptr, nullptr,
                                             &matched_2d_old[matched_2d_old.size() - n].x, &matched_2d_old_norm[matched_2d_old_norm.size() - n].x, nullptr), "lmono_keyframes_match");
}

template <typename T> static void reduceVector(std::vector<T> &v, const std::vector<unsigned char> &status)
{
    size_t j = 0;
    for (size_t i = 0; i < v.size(); i++) if (status[i]) v[j++] = v[i];
    v.resize(j);
}

bool KeyFrame::findConnection(const KeyFrame *old_kf, std::vector<Point2f> &matched_2d_cur, std::vector<Point2f> &matched_2d_old, std::vector<Point2f> &matched_2d_cur_norm,
                              std::vector<Point2f> &matched_2d_old_norm, std::vector<Point3f> &matched_3d, std::vector<int> &matched_id)
{
    std::vector<unsigned char> status;
    matched_3d = point_3d; matched_2d_cur = point_2d_uv; matched_2d_cur_norm = point_2d_norm; matched_id = point_id;      // :383-386
    matched_2d_old.clear(); matched_2d_old_norm.clear();
    searchByBRIEFDes(matched_2d_old, matched_2d_old_norm, status, old_kf);
    reduceVector(matched_2d_cur, status); reduceVector(matched_2d_old, status); reduceVector(matched_2d_cur_norm, status);
    reduceVector(matched_2d_old_norm, status); reduceVector(matched_3d, status); reduceVector(matched_id, status);
    return (int)matched_2d_cur.size() > MIN_BRIEF_LOOP_NUM;                                                               // :557
}

} // namespace lmono_host
