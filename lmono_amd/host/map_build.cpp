// lmono_amd/host/map_build.cpp -- the map_builder node's loop (mono_lidar_mapping/src/map_build_node.cc:140-236) over files:
// for every frame k: scan <seq>/velodyne/%06d.bin + image <seq>/image_bgr/%06d.bgr (raw BGR8, width * height * 3 bytes: this
// image has no PNG decoder) + pose line k of a trajectory file ("stamp x y z qx qy qz qw", the format the estimator writes)
// -> MapBuilder::associateToMap -> processMapping; writes <out>/rgb_map<index>.ply every 10 frames and the timing log
// <out>/mapping_recorder.txt, and dumps the products of the last frame (<out>/depth_last.u8, <out>/cloud_cam_last.bin,
// <out>/cloud_world_last.bin) for inspection.
//   map_build <sequence_dir> <trajectory.txt> <out_dir> [n_frames] [width height fx fy cx cy] [submap=N:CORRECTED_TRAJECTORY[:LEAF_SUB]] [sor=K:MULT[:CELL:RINGS]] [icp=D[:ITERS[:EPS]]] [voxel=LEAF[:MAX_VOXELS[:GROW_LIMIT]]] [normals=R[:MIN[:CELL:RINGS]]]
// With normals= behind voxel= the finished voxel map's points get their surface normals and curvature within radius R (MIN 3 neighbours,
// the default grid unless given; no viewpoint), written as <out>/rgb_map_voxel_normals.ply beside rgb_map_voxel.ply: the same points in the device's order.
// With the voxel= argument every frame is also folded into a voxel-grid map, written at the end as
// <out>/rgb_map_voxel.ply; without it nothing changes.  With a GROW_LIMIT the map starts at MAX_VOXELS and grows on the device up to that limit, and so
// do the composed map and the submaps (each from MAX_VOXELS), whose tables are shrunk to their content once closed.  With sor= in front of it every frame passes the statistical outlier removal
// (CELL 0.1 and RINGS 8 unless given) on its way into that map.  With icp= directly in front of voxel= every frame but the first is aligned against that map by
// point-to-point ICP (max correspondence distance D, ITERS 50 and EPS 1e-8 unless given) before it is folded in, and an
// "ICP <frame> iterations <k> status <s> N <pairs> mse <m^2>" line is printed per frame (a frame that was not aligned: iterations 0, status 3).  With submap= in front of those every N frames also go into a
// submap of their own (LEAF_SUB 0.05 unless given), and at the end the submaps are composed under the poses of CORRECTED_TRAJECTORY (same format,
// one line per frame: a loop-closed trajectory) into <out>/rgb_map_global.ply at the voxel= leaf.
#include "kitti_io.hpp"
#include "lmono_host.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace lmono_host;

static bool read_file(const std::string &path, std::vector<uint8_t> &out, size_t expect)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    out.resize(expect);
    const bool ok = std::fread(out.data(), 1, expect, f) == expect && std::fgetc(f) == EOF;
    std::fclose(f);
    return ok;
}

template <typename T> static bool dump(const std::string &path, const std::vector<T> &v)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv)
{
    float nrm_r = 0.0f, nrm_cell = 0.0f;
    int nrm_min = 3, nrm_rings = 2;
    if (argc > 5 && std::strncmp(argv[argc - 1], "normals=", 8) == 0) {
        const int got = std::sscanf(argv[argc - 1] + 8, "%f:%d:%f:%d", &nrm_r, &nrm_min, &nrm_cell, &nrm_rings);
        if ((got != 1 && got != 2 && got != 4) || !(nrm_r > 0.0f) || nrm_min < 3 || std::strncmp(argv[argc - 2], "voxel=", 6) != 0) {
            std::fprintf(stderr, "map_build: normals=R[:MIN[:CELL:RINGS]] needs R > 0, MIN >= 3 and a voxel= argument directly in front of it\n");
            return 2;
        }
        argc--;
    }
    float voxel_leaf = 0.0f;
    long long voxel_max = 1 << 22, voxel_grow = 0;
    if (argc > 4 && std::strncmp(argv[argc - 1], "voxel=", 6) == 0) {
        char *end = nullptr;
        voxel_leaf = std::strtof(argv[argc - 1] + 6, &end);
        if (end && *end == ':') {
            voxel_max = std::strtoll(end + 1, &end, 10);
            if (end && *end == ':') voxel_grow = std::atoll(end + 1);
        }
        if (!(voxel_leaf > 0.0f)) { std::fprintf(stderr, "map_build: voxel=LEAF[:MAX_VOXELS[:GROW_LIMIT]] needs a leaf > 0\n"); return 2; }
        argc--;
    }
    float icp_d = 0.0f;
    int icp_iters = 50;
    double icp_eps = 1e-8;
    if (argc > 4 && std::strncmp(argv[argc - 1], "icp=", 4) == 0) {
        const int got = std::sscanf(argv[argc - 1] + 4, "%f:%d:%lf", &icp_d, &icp_iters, &icp_eps);
        if (got < 1 || !(icp_d > 0.0f) || icp_iters < 1 || !(icp_eps >= 0.0) || !(voxel_leaf > 0.0f)) { std::fprintf(stderr, "map_build: icp=D[:ITERS[:EPS]] needs D > 0, ITERS >= 1, EPS >= 0 and a voxel= argument behind it\n"); return 2; }
        argc--;
    }
    int sor_k = 0, sor_rings = 8;
    double sor_mul = 1.0;
    float sor_cell = 0.1f;
    if (argc > 4 && std::strncmp(argv[argc - 1], "sor=", 4) == 0) {
        const int got = std::sscanf(argv[argc - 1] + 4, "%d:%lf:%f:%d", &sor_k, &sor_mul, &sor_cell, &sor_rings);
        if ((got != 2 && got != 4) || sor_k < 1 || !(voxel_leaf > 0.0f)) { std::fprintf(stderr, "map_build: sor=K:MULT[:CELL:RINGS] needs K >= 1 and a voxel= argument behind it\n"); return 2; }
        argc--;
    }
    int sub_n = 0;
    float sub_leaf = 0.05f;
    std::string sub_traj;
    if (argc > 4 && std::strncmp(argv[argc - 1], "submap=", 7) == 0) {
        char *end = nullptr;
        sub_n = (int)std::strtol(argv[argc - 1] + 7, &end, 10);
        if (sub_n < 1 || !end || *end != ':' || !(voxel_leaf > 0.0f)) { std::fprintf(stderr, "map_build: submap=N:CORRECTED_TRAJECTORY[:LEAF_SUB] needs N >= 1 and a voxel= argument behind it\n"); return 2; }
        sub_traj = end + 1;
        const size_t colon = sub_traj.rfind(':');
        if (colon != std::string::npos && colon + 1 < sub_traj.size()) {      // a trailing :LEAF_SUB, when what follows the last colon is a number
            char *e2 = nullptr;
            const float v = std::strtof(sub_traj.c_str() + colon + 1, &e2);
            if (e2 && *e2 == 0) {
                if (!(v > 0.0f)) { std::fprintf(stderr, "map_build: submap= needs a LEAF_SUB > 0\n"); return 2; }
                sub_leaf = v; sub_traj.resize(colon);
            }
        }
        argc--;
    }
    if (argc < 4) { std::fprintf(stderr, "usage: map_build <sequence_dir> <trajectory.txt> <out_dir> [n_frames] [width height fx fy cx cy] [submap=N:CORRECTED_TRAJECTORY[:LEAF_SUB]] [sor=K:MULT[:CELL:RINGS]] [icp=D[:ITERS[:EPS]]] [voxel=LEAF[:MAX_VOXELS[:GROW_LIMIT]]] [normals=R[:MIN[:CELL:RINGS]]]\n"); return 2; }
    const std::string seq = argv[1], traj = argv[2], out = argv[3];
    int n_frames = argc > 4 ? std::atoi(argv[4]) : -1;
    lmono_camera cam = { 1241, 376, 718.856, 718.856, 607.1928, 185.2157, 0, 0, 0, 0, 5, 0, 0 };   // kitti00_cam.yaml, kitti_map_config_00.yaml
    if (argc > 10) { cam.width = std::atoi(argv[5]); cam.height = std::atoi(argv[6]); cam.fx = std::atof(argv[7]); cam.fy = std::atof(argv[8]); cam.cx = std::atof(argv[9]); cam.cy = std::atof(argv[10]); }
    // camera-from-LiDAR extrinsic of the KITTI rig (camera x right, y down, z forward; p_l = rlc p_c + tlc)
    const double rlc[9] = { 0, 0, 1, -1, 0, 0, 0, -1, 0 }, tlc[3] = { 0.27, 0.0, -0.08 };
    std::vector<std::array<double, 8>> poses;
    {
        FILE *f = std::fopen(traj.c_str(), "r");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", traj.c_str()); return 1; }
        std::array<double, 8> p;
        while (std::fscanf(f, "%lf %lf %lf %lf %lf %lf %lf %lf", &p[0], &p[1], &p[2], &p[3], &p[4], &p[5], &p[6], &p[7]) == 8) poses.push_back(p);
        std::fclose(f);
    }
    if (n_frames < 0 || n_frames > (int)poses.size()) n_frames = (int)poses.size();
    std::vector<std::array<double, 7>> corrected;
    if (sub_n > 0) {
        FILE *f = std::fopen(sub_traj.c_str(), "r");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", sub_traj.c_str()); return 1; }
        std::array<double, 8> p;
        while (std::fscanf(f, "%lf %lf %lf %lf %lf %lf %lf %lf", &p[0], &p[1], &p[2], &p[3], &p[4], &p[5], &p[6], &p[7]) == 8) corrected.push_back({ p[1], p[2], p[3], p[4], p[5], p[6], p[7] });
        std::fclose(f);
        if ((int)corrected.size() < n_frames) { std::fprintf(stderr, "map_build: %s has fewer poses than frames\n", sub_traj.c_str()); return 1; }
    }
    try {
        HipContext hip(0);
        MapBuilder map_builder(hip, cam, true, out);
        if (voxel_leaf > 0.0f) map_builder.setVoxelMap(voxel_leaf, voxel_max, voxel_grow);
        if (sor_k > 0) map_builder.setOutlierFilter(sor_k, sor_mul, sor_cell, sor_rings);
        if (icp_d > 0.0f) map_builder.setAligner(icp_d, icp_iters, icp_eps);
        if (nrm_r > 0.0f) map_builder.setNormals(nrm_r, nrm_min, nrm_cell, nrm_rings);
        if (sub_n > 0 && voxel_grow > 0) map_builder.setSubmaps(sub_n, sub_leaf, voxel_max, voxel_grow, /*compact_closed=*/true);
        else if (sub_n > 0) map_builder.setSubmaps(sub_n, sub_leaf);
        MappingLog recorder(out + "/mapping_recorder.txt");
        if (!recorder.ok()) { std::fprintf(stderr, "cannot write into %s\n", out.c_str()); return 1; }
        std::vector<uint8_t> image;
        for (int k = 0; k < n_frames; k++) {
            std::vector<float> xyzi;
            const long n = read_velodyne_bin(velodyne_path(seq, k), xyzi);
            char name[64];
            std::snprintf(name, sizeof name, "/image_bgr/%06d.bgr", k);
            if (n < 0 || !read_file(seq + name, image, (size_t)cam.width * cam.height * 3)) { std::fprintf(stderr, "frame %d unreadable\n", k); return 1; }
            const double *p = poses[(size_t)k].data();
            const auto t0 = std::chrono::steady_clock::now();
            const int m = map_builder.associateToMap(p + 4, p + 1, xyzi.data(), (int)n, rlc, tlc, image.data(), p[0]);
            recorder.write(p[0], std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            const std::string written = map_builder.processMapping();
            std::printf("FRAME %d points_in %ld points_out %d%s%s\n", k, n, m, written.empty() ? "" : " wrote ", written.c_str());
            if (icp_d > 0.0f) {
                const int64_t *st = map_builder.alignerStats();
                std::printf("ICP %d iterations %lld status %lld N %lld mse %.9g\n", k, (long long)st[4], (long long)st[5], (long long)st[6], st[6] > 0 ? (double)st[7] / (double)st[6] / 16777216.0 : 0.0);
            }
            if (k == n_frames - 1) {
                if (!dump(out + "/depth_last.u8", map_builder.depthMap()) || !dump(out + "/cloud_cam_last.bin", map_builder.rgbCloud(0))) return 1;
                if (written.empty() && !dump(out + "/cloud_world_last.bin", map_builder.rgbCloud(1))) return 1;
            }
        }
        if (voxel_leaf > 0.0f) {
            const std::vector<lmono_point_rgb> v = map_builder.voxelMap();
            const std::string path = out + "/rgb_map_voxel.ply";
            if (!write_ply_binary(path, reinterpret_cast<const PointRgb *>(v.data()), v.size())) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
        }
        if (nrm_r > 0.0f) {
            std::vector<lmono_point_rgb> v;
            std::vector<lmono_normal> nv;
            map_builder.voxelNormals(v, nv);
            static_assert(sizeof(lmono_normal) == sizeof(PlyNormal), "the record is the file's");
            const std::string path = out + "/rgb_map_voxel_normals.ply";
            if (!write_ply_binary_normals(path, reinterpret_cast<const PointRgb *>(v.data()), reinterpret_cast<const PlyNormal *>(nv.data()), v.size())) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
        }
        if (sub_n > 0) {
            const std::vector<lmono_point_rgb> v = map_builder.composeMap(corrected);
            const std::string path = out + "/rgb_map_global.ply";
            if (!write_ply_binary(path, reinterpret_cast<const PointRgb *>(v.data()), v.size())) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "map_build: %s\n", e.what());
        return 1;
    }
    return 0;
}
