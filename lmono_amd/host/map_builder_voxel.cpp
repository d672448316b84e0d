// lmono_amd/host/map_builder_voxel.cpp -- MapBuilder::setVoxelMap / voxelMap: the voxel-grid step of processMapping (the
// pcl::VoxelGrid block the reference carries commented out, Map_Builder.cc:82-98) behind lmono_voxel_map_*.
#include "lmono_host.hpp"

#include <stdexcept>

namespace lmono_host {

void MapBuilder::setVoxelMap(float leaf, int64_t max_voxels)
{
    lmono_voxel_map *vm = lmono_voxel_map_create(hip_.get(), leaf, max_voxels);
    if (!vm) throw std::runtime_error(std::string("lmono_voxel_map_create: ") + lmono_last_error(hip_.get()));
    vm_ = std::shared_ptr<lmono_voxel_map>(vm, lmono_voxel_map_destroy);
    fold_ = [this] {
        lmono_voxel_map *m = vm_.get();
        if (lmono_sor *f = sor_.get()) {                                   // :24-29 in front of :82-98
            hip_.check(lmono_sor_filter_frames(hip_.get(), 1, &f, &mb_, nullptr), "lmono_sor_filter_frames");
            hip_.check(lmono_voxel_map_insert_filtered(hip_.get(), 1, &m, &f, nullptr), "lmono_voxel_map_insert_filtered");
            return;
        }
        hip_.check(lmono_voxel_map_insert_frames(hip_.get(), 1, &m, &mb_, nullptr), "lmono_voxel_map_insert_frames");
    };
}

void MapBuilder::setOutlierFilter(int mean_k, double stddev_mul, float cell, int max_rings)
{
    lmono_sor *f = lmono_sor_create(hip_.get(), (int64_t)cam_.width * cam_.height, mean_k, stddev_mul, cell, max_rings);
    if (!f) throw std::runtime_error(std::string("lmono_sor_create: ") + lmono_last_error(hip_.get()));
    sor_ = std::shared_ptr<lmono_sor>(f, lmono_sor_destroy);
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
