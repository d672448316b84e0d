// lmono_amd/host/map_builder_voxel.cpp -- MapBuilder::setVoxelMap / voxelMap: the voxel-grid step of processMapping (the
// pcl::VoxelGrid block the reference carries commented out, Map_Builder.cc:82-98) behind lmono_voxel_map_*.
#include "lmono_host.hpp"

#include <cmath>
#include <stdexcept>

namespace lmono_host {

// a voxel map of max_voxels that grows up to grow_limit (0: fixed size)
std::shared_ptr<lmono_voxel_map> MapBuilder::newVoxelMap(float leaf, int64_t max_voxels, int64_t grow_limit)
{
    lmono_voxel_map *vm = lmono_voxel_map_create(hip_.get(), leaf, max_voxels);
    if (!vm) throw std::runtime_error(std::string("lmono_voxel_map_create: ") + lmono_last_error(hip_.get()));
    std::shared_ptr<lmono_voxel_map> p(vm, lmono_voxel_map_destroy);
    if (grow_limit) hip_.check(lmono_voxel_map_set_growth(hip_.get(), vm, grow_limit), "lmono_voxel_map_set_growth");
    return p;
}

void MapBuilder::setVoxelMap(float leaf, int64_t max_voxels, int64_t grow_limit)
{
    vm_ = newVoxelMap(leaf, max_voxels, grow_limit);
    vm_leaf_ = leaf; vm_max_ = max_voxels; vm_grow_ = grow_limit;
    fold_ = [this] {
        lmono_voxel_map *m = vm_.get();
        lmono_voxel_map *sub = submapForFrame();                           // the same frame into its submap
        lmono_icp *a = icp_.get();
        for (int64_t &v : icp_stats_) v = 0;
        icp_stats_[5] = 3;                                               // no align ran: no iteration, no pairs, as an align of nothing reports
        const bool align = a && lmono_voxel_map_size(hip_.get(), m) > 0;  // :31-59 between them; an empty map is no target
        if (align) hip_.check(lmono_icp_set_target_map(hip_.get(), a, m), "lmono_icp_set_target_map");
        if (lmono_sor *f = sor_.get()) {                                   // :24-29 in front of :82-98
            hip_.check(lmono_sor_filter_frames(hip_.get(), 1, &f, &mb_, nullptr), "lmono_sor_filter_frames");
            if (align) hip_.check(lmono_icp_align_filtered(hip_.get(), 1, &a, &f, icp_stats_), "lmono_icp_align_filtered");
            else {
                hip_.check(lmono_voxel_map_insert_filtered(hip_.get(), 1, &m, &f, nullptr), "lmono_voxel_map_insert_filtered");
                if (sub) hip_.check(lmono_voxel_map_insert_filtered(hip_.get(), 1, &sub, &f, nullptr), "lmono_voxel_map_insert_filtered");
                return;
            }
        } else if (align) hip_.check(lmono_icp_align_frames(hip_.get(), 1, &a, &mb_, icp_stats_), "lmono_icp_align_frames");
        if (align) {
            hip_.check(lmono_voxel_map_insert_aligned(hip_.get(), 1, &m, &a, nullptr), "lmono_voxel_map_insert_aligned");
            if (sub) hip_.check(lmono_voxel_map_insert_aligned(hip_.get(), 1, &sub, &a, nullptr), "lmono_voxel_map_insert_aligned");
            return;
        }
        hip_.check(lmono_voxel_map_insert_frames(hip_.get(), 1, &m, &mb_, nullptr), "lmono_voxel_map_insert_frames");
        if (sub) hip_.check(lmono_voxel_map_insert_frames(hip_.get(), 1, &sub, &mb_, nullptr), "lmono_voxel_map_insert_frames");
    };
}

void MapBuilder::setSubmaps(int frames_per_submap, float leaf_sub, int64_t max_voxels_sub, int64_t grow_limit_sub, bool compact_closed)
{
    if (!vm_) throw std::runtime_error("MapBuilder::setSubmaps: setVoxelMap first (composeMap writes at its leaf)");
    if (frames_per_submap < 1 || !(leaf_sub > 0.0f) || max_voxels_sub < 1) throw std::runtime_error("MapBuilder::setSubmaps: frames_per_submap >= 1, leaf_sub > 0, max_voxels_sub >= 1");
    sub_ = Submaps();
    sub_.per = frames_per_submap; sub_.leaf = leaf_sub; sub_.max_voxels = max_voxels_sub;
    sub_.grow_limit = grow_limit_sub; sub_.compact_closed = compact_closed;
}

// shrink the submaps not yet shrunk (all closed when this is called) to what they hold: one batched reserve
void MapBuilder::compactSubmaps()
{
    if (!sub_.compact_closed || sub_.compacted == sub_.maps.size()) return;
    std::vector<lmono_voxel_map *> maps;
    std::vector<int64_t> sizes;
    for (size_t s = sub_.compacted; s < sub_.maps.size(); s++) {
        const int64_t n = lmono_voxel_map_size(hip_.get(), sub_.maps[s].get());
        hip_.check(n < 0 ? (int)n : 0, "lmono_voxel_map_size");
        maps.push_back(sub_.maps[s].get());
        sizes.push_back(n > 1 ? n : 1);
    }
    hip_.check(lmono_voxel_map_reserve(hip_.get(), (int)maps.size(), maps.data(), sizes.data()), "lmono_voxel_map_reserve");
    sub_.compacted = sub_.maps.size();
}

lmono_voxel_map *MapBuilder::submapForFrame()
{
    if (sub_.per == 0) return nullptr;
    if (sub_.frames % sub_.per == 0) {
        compactSubmaps();
        sub_.maps.push_back(newVoxelMap(sub_.leaf, sub_.max_voxels, sub_.grow_limit));
        sub_.anchor_frame.push_back(sub_.frames);
        std::array<double, 7> a;
        for (int k = 0; k < 7; k++) a[(size_t)k] = last_tq_[k];
        sub_.anchor_tq.push_back(a);
    }
    sub_.frames++;
    return sub_.maps.back().get();
}

// T_corrected * T_inserted^-1 (the formula of lmono_amd.pose_delta, operation for operation): with q / |q| = (x, y, z, w) and R(q) the usual
// rotation matrix, D_R = R_c R_i^T and D_t = t_c - D_R t_i, every sum left to right
static void pose_matrix(const double tq[7], double R[9])
{
    const double n = std::sqrt(((tq[3] * tq[3] + tq[4] * tq[4]) + tq[5] * tq[5]) + tq[6] * tq[6]);
    const double x = tq[3] / n, y = tq[4] / n, z = tq[5] / n, w = tq[6] / n;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - z * w); R[2] = 2.0 * (x * z + y * w);
    R[3] = 2.0 * (x * y + z * w); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - x * w);
    R[6] = 2.0 * (x * z - y * w); R[7] = 2.0 * (y * z + x * w); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

void MapBuilder::poseDelta(const double inserted_tq[7], const double corrected_tq[7], double D[12])
{
    double Ri[9], Rc[9];
    pose_matrix(inserted_tq, Ri);
    pose_matrix(corrected_tq, Rc);
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) D[4 * a + b] = (Rc[3 * a] * Ri[3 * b] + Rc[3 * a + 1] * Ri[3 * b + 1]) + Rc[3 * a + 2] * Ri[3 * b + 2];
        D[4 * a + 3] = corrected_tq[a] - ((D[4 * a] * inserted_tq[0] + D[4 * a + 1] * inserted_tq[1]) + D[4 * a + 2] * inserted_tq[2]);
    }
}

std::vector<lmono_point_rgb> MapBuilder::composeMap(const std::vector<std::array<double, 7>> &corrected_tq)
{
    std::vector<lmono_point_rgb> out;
    if (sub_.per == 0) throw std::runtime_error("MapBuilder::composeMap: setSubmaps first");
    if ((int)corrected_tq.size() < sub_.frames) throw std::runtime_error("MapBuilder::composeMap: one corrected pose per frame folded");
    const size_t n = sub_.maps.size();
    std::vector<lmono_voxel_map *> srcs(n);
    std::vector<double> T(12 * n);
    for (size_t s = 0; s < n; s++) {
        srcs[s] = sub_.maps[s].get();
        poseDelta(sub_.anchor_tq[s].data(), corrected_tq[(size_t)sub_.anchor_frame[s]].data(), &T[12 * s]);
    }
    compactSubmaps();
    const std::shared_ptr<lmono_voxel_map> global = newVoxelMap(vm_leaf_, vm_max_, vm_grow_);
    lmono_voxel_map *g = global.get();
    hip_.check(lmono_voxel_map_compose(hip_.get(), g, (int)n, srcs.data(), T.data(), nullptr), "lmono_voxel_map_compose");
    const int64_t m = lmono_voxel_map_read(hip_.get(), g, nullptr, 0);
    hip_.check(m < 0 ? (int)m : 0, "lmono_voxel_map_read");
    out.resize((size_t)m);
    if (m > 0) hip_.check(lmono_voxel_map_read(hip_.get(), g, out.data(), m) < 0 ? -1 : 0, "lmono_voxel_map_read");
    return out;
}

void MapBuilder::setOutlierFilter(int mean_k, double stddev_mul, float cell, int max_rings)
{
    lmono_sor *f = lmono_sor_create(hip_.get(), (int64_t)cam_.width * cam_.height, mean_k, stddev_mul, cell, max_rings);
    if (!f) throw std::runtime_error(std::string("lmono_sor_create: ") + lmono_last_error(hip_.get()));
    sor_ = std::shared_ptr<lmono_sor>(f, lmono_sor_destroy);
}

void MapBuilder::setAligner(float max_corr, int max_iter, double eps, double mse_eps)
{
    if (!vm_) throw std::runtime_error("MapBuilder::setAligner: setVoxelMap first (the map is the target)");
    // the target is the map: as many points as it may ever hold voxels; the grid at its defaults (lmono_icp_default_cell, 2 rings)
    lmono_icp *a = lmono_icp_create(hip_.get(), (int64_t)cam_.width * cam_.height, vm_grow_ > vm_max_ ? vm_grow_ : vm_max_, max_corr, max_iter, eps, mse_eps, lmono_icp_default_cell(max_corr), 2);
    if (!a) throw std::runtime_error(std::string("lmono_icp_create: ") + lmono_last_error(hip_.get()));
    icp_ = std::shared_ptr<lmono_icp>(a, lmono_icp_destroy);
}

void MapBuilder::setNormals(float radius, int min_neighbours, float cell, int max_rings)
{
    if (!vm_) throw std::runtime_error("MapBuilder::setNormals: setVoxelMap first (the map's points get the normals)");
    // one point per voxel: as many points as the map may ever hold voxels
    lmono_normals *s = lmono_normals_create(hip_.get(), vm_grow_ > vm_max_ ? vm_grow_ : vm_max_, radius, min_neighbours, cell > 0.0f ? cell : lmono_normals_default_cell(radius), max_rings);
    if (!s) throw std::runtime_error(std::string("lmono_normals_create: ") + lmono_last_error(hip_.get()));
    nrm_ = std::shared_ptr<lmono_normals>(s, lmono_normals_destroy);
}

void MapBuilder::voxelNormals(std::vector<lmono_point_rgb> &points, std::vector<lmono_normal> &normals)
{
    points.clear(); normals.clear();
    if (!nrm_) throw std::runtime_error("MapBuilder::voxelNormals: setNormals first");
    lmono_normals *s = nrm_.get();
    hip_.check(lmono_normals_compute_map(hip_.get(), s, vm_.get(), nullptr, nullptr), "lmono_normals_compute_map");
    const int64_t n = lmono_normals_read(hip_.get(), s, nullptr, nullptr, 0);
    hip_.check(n < 0 ? (int)n : 0, "lmono_normals_read");
    points.resize((size_t)n); normals.resize((size_t)n);
    if (n == 0) return;
    hip_.check(lmono_normals_read(hip_.get(), s, normals.data(), nullptr, n) < 0 ? -1 : 0, "lmono_normals_read");
    hip_.check(lmono_normals_cloud(hip_.get(), s, points.data(), n) < 0 ? -1 : 0, "lmono_normals_cloud");
}

std::vector<lmono_point_rgb> MapBuilder::voxelMap()
{
    std::vector<lmono_point_rgb> out;
    if (!vm_) return out;
    const int64_t n = lmono_voxel_map_read(hip_.get(), vm_.get(), nullptr, 0);
    hip_.check(n < 0 ? (int)n : 0, "lmono_voxel_map_read");
    out.resize((size_t)n);
    if (n > 0) hip_.check(lmono_voxel_map_read(hip_.get(), vm_.get(), out.data(), n) < 0 ? -1 : 0, "lmono_voxel_map_read");
    return out;
}

} // namespace lmono_host
