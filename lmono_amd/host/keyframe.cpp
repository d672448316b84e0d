// lmono_amd/host/keyframe.cpp -- see keyframe.hpp
#include "keyframe.hpp"
#include "../csrc/pnp.hip"      // plain C++ here: pnp_guess, pnp_after
#include <cmath>
#include <cstdlib>
#include <cstring>
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

void KeyFrame::PnPRANSAC(const std::vector<Point2f> &matched_2d_old_norm, const std::vector<Point3f> &matched_3d, std::vector<unsigned char> &status,
                         double *PnP_T_old, double *PnP_q_old, uint32_t key)
{
    if (matched_2d_old_norm.size() != matched_3d.size()) throw std::runtime_error("PnPRANSAC: matched_2d_old_norm and matched_3d differ in length");
    const int32_t m = (int32_t)matched_3d.size();
    lmono::PnpPose G;
    lmono::pnp_guess(origin_vio_tq, ex_tq, G);                                   // :308-312
    double guess[7] = { G.t[0], G.t[1], G.t[2], G.q[0], G.q[1], G.q[2], G.q[3] }, pose[7];
    const size_t at = status.size();
    status.resize(at + (size_t)m + 1);                                           // + 1: an address to hand over when m is 0
    store_.hip().check(lmono_pnp_ransac(store_.hip().get(), &pnp_params, 1, &m, m ? &matched_3d[0].x : nullptr, m ? &matched_2d_old_norm[0].x : nullptr, guess, &key,
                                        &status[at], pose, nullptr), "lmono_pnp_ransac");
    status.resize(at + (size_t)m);
    lmono::PnpLoop L;
    lmono::pnp_after(pose, origin_vio_tq, ex_tq, 0.0, 0.0, L);                   // :341-350
    for (int e = 0; e < 3; e++) PnP_T_old[e] = L.t_old[e];
    for (int e = 0; e < 4; e++) PnP_q_old[e] = L.q_old[e];
}

bool KeyFrame::findConnection(const KeyFrame *old_kf)
{
    const size_t n = point_2d_uv.size();
    if (point_3d.size() != n || point_2d_norm.size() != n || point_id.size() != n) throw std::runtime_error("findConnection: point_3d, point_2d_norm and point_id must match point_2d_uv");
    const int32_t old_index = old_kf->store_index;
    std::vector<unsigned char> status(n + 1);
    std::vector<Point2f> old_norm(n + 1);
    int32_t brief = 0, inliers = 0;
    uint8_t has = 0;
    double info[8], channel[15];
    lmono_ctx *c = store_.hip().get();
    store_.hip().check(lmono_keyframes_verify(c, store_.get(), store_index, 1, &old_index, n ? &point_3d[0].x : nullptr, origin_vio_tq, ex_tq, old_kf->T_w_i_tq, &pnp_params,
                                              &brief, &inliers, status.data(), nullptr, info, &has, channel, nullptr, nullptr, nullptr), "lmono_keyframes_verify");
    matched_brief = brief; matched_pnp = inliers;
    if (!has) return false;                                                      // :689-690
    // the matched old points of the survivors: the search's output for this pair, reduced by the status after both reductions
    store_.hip().check(lmono_keyframes_match(c, store_.get(), store_index, 1, &old_index, nullptr, nullptr, nullptr, nullptr, &old_norm[0].x, nullptr), "lmono_keyframes_match");
    status.resize(n); old_norm.resize(n);
    point_loop_2d_norm = point_2d_norm; point_old_2d_norm = old_norm; point_loop_id = point_id;              // :590-592
    reduceVector(point_loop_2d_norm, status); reduceVector(point_old_2d_norm, status); reduceVector(point_loop_id, status);
    has_loop = true; loop_index = old_kf->index;                                 // :636-637
    for (int e = 0; e < 8; e++) loop_info[e] = info[e];
    published.stamp = time_stamp; published.points.clear();
    for (size_t i = 0; i < point_old_2d_norm.size(); i++) published.points.push_back({ point_old_2d_norm[i].x, point_old_2d_norm[i].y, (float)point_loop_id[i] });
    for (int e = 0; e < 14; e++) published.t_q_index[e] = channel[e];
    published.t_q_index[14] = (double)index;                                     // :681: the keyframe's own index, not its slot in the store
    return true;
}

LoopDetector::LoopDetector(KeyFrameStore &store, int loop_search_gap, double loop_search_time)
    : LOOP_SEARCH_GAP(loop_search_gap), LOOP_SEARCH_TIME(loop_search_time), store_(store) {}

LoopDetector::~LoopDetector()
{
    if (voc_) lmono_brief_vocabulary_destroy(voc_);         // the store keeps the device tree for as long as it is attached
}

void LoopDetector::loadVocabulary(const std::string &voc_path)
{
    std::ifstream in(voc_path, std::ios::binary);
    if (!in) throw std::runtime_error("loadVocabulary: cannot open " + voc_path);
    int32_t head[6];
    in.read((char *)head, sizeof(head));
    if (!in || head[4] < 0 || head[4] > 16777215 || head[5] < 0 || head[5] > 16777215) throw std::runtime_error("loadVocabulary: " + voc_path + " has no vocabulary header");
    const size_t n = (size_t)head[4], nw = (size_t)head[5];
    std::vector<char> nodes(n * 48), words(nw * 8);
    in.read(nodes.data(), (std::streamsize)nodes.size());
    in.read(words.data(), (std::streamsize)words.size());
    if ((size_t)in.gcount() != words.size() || !in) throw std::runtime_error("loadVocabulary: " + voc_path + " is shorter than its header says");
    std::vector<int32_t> node_id(n), parent_id(n), word_node(nw), word_id(nw);
    std::vector<double> weight(n);
    std::vector<uint32_t> desc(n * 8);
    for (size_t r = 0; r < n; r++) {
        const char *p = nodes.data() + r * 48;
        std::memcpy(&node_id[r], p, 4); std::memcpy(&parent_id[r], p + 4, 4); std::memcpy(&weight[r], p + 8, 8); std::memcpy(&desc[r * 8], p + 16, 32);
    }
    for (size_t r = 0; r < nw; r++) { std::memcpy(&word_node[r], words.data() + r * 8, 4); std::memcpy(&word_id[r], words.data() + r * 8 + 4, 4); }
    lmono_ctx *c = store_.hip().get();
    lmono_brief_vocabulary *voc = lmono_brief_vocabulary_create(c, head[0], head[1], head[2], head[3], head[4], node_id.data(), parent_id.data(), weight.data(), desc.data(),
                                                                head[5], word_node.data(), word_id.data());
    if (!voc) throw std::runtime_error(std::string("lmono_brief_vocabulary_create: ") + lmono_last_error(c));
    const int rc = lmono_keyframes_set_vocabulary(c, store_.get(), voc);                     // db.setVocabulary(*voc, false, 0)
    if (rc != LMONO_OK) { lmono_brief_vocabulary_destroy(voc); store_.hip().check(rc, "lmono_keyframes_set_vocabulary"); }
    if (voc_) lmono_brief_vocabulary_destroy(voc_);
    voc_ = voc;
}

int LoopDetector::detectLoop(KeyFrame *keyframe, int frame_index)
{
    (void)frame_index;                                   // the database entry of a keyframe is its slot in the store
    int loop_slot = -1, n = 0;
    int32_t id[4];
    double score[4];
    store_.hip().check(lmono_keyframes_detect_loop(store_.hip().get(), store_.get(), keyframe->store_index, LOOP_SEARCH_GAP, &loop_slot, &n, id, score), "lmono_keyframes_detect_loop");
    ret_id.assign(id, id + n); ret_score.assign(score, score + n);
    if (loop_slot == -1) return -1;
    for (KeyFrame *kf : keyframelist) if (kf->store_index == loop_slot) return kf->index;
    return -1;
}

int LoopDetector::addKeyFrame(KeyFrame *cur_kf, bool flag_detect_loop)
{
    int loop_index = -1;
    if (flag_detect_loop) loop_index = detectLoop(cur_kf, cur_kf->index);
    // else addKeyFrameIntoVoc: the keyframe is in the store already, its BoW vector is built when a query first needs it
    if (loop_index != -1) {
        KeyFrame *old_kf = getKeyFrame(loop_index);
        if (old_kf && std::fabs(cur_kf->time_stamp - old_kf->time_stamp) > LOOP_SEARCH_TIME) {          // :73
            if (cur_kf->findConnection(old_kf)) {
                loop_index = old_kf->index;
                double old_tq[7], cur_tq[7], R_old[9];
                old_kf->getVioPose(old_tq);
                const double *rel_t = cur_kf->loop_info;                                                 // getLoopRelativeT / Q (w x y z)
                const double rel_q[4] = { cur_kf->loop_info[4], cur_kf->loop_info[5], cur_kf->loop_info[6], cur_kf->loop_info[3] };
                lmono::pnp_rot(old_tq + 3, R_old);
                lmono::pnp_apply(R_old, old_tq, rel_t, cur_tq);                                          // w_P_cur = w_R_old * relative_t + w_P_old
                lmono::pnp_qmul(old_tq + 3, rel_q, cur_tq + 3);                                          // w_R_cur = w_R_old * relative_q
                cur_kf->updateVioPose(cur_tq);
            } else loop_index = -1;
        }
    }
    keyframelist.push_back(cur_kf);
    return loop_index;
}

KeyFrame *LoopDetector::getKeyFrame(int index)
{
    for (KeyFrame *kf : keyframelist) if (kf->index == index) return kf;
    return nullptr;
}

} // namespace lmono_host
