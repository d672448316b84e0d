"""The host mirror's normals (MapBuilder::setNormals) through the map_build program: the finished voxel map's points with their
normals and curvature in rgb_map_voxel_normals.ply, equal to SurfaceNormals.compute_map over the same frames in Python."""
import os
import subprocess

import numpy as np
import pytest

from tests import colour_cases as CC
from tests import normals_ref as R

pytestmark = pytest.mark.gpu


def _by_point(p):
    return np.lexsort((p["bgra"], p["z"], p["y"], p["x"]))


def test_cpp_map_build_writes_the_voxel_maps_normals(gpu_ctx, tmp_path):
    """map_build ... voxel=0.1 normals=0.3 writes rgb_map_voxel_normals.ply beside rgb_map_voxel.ply: the same points (in the device's order), and
    per point the record the Python chain computes."""
    import lmono_amd
    from lmono_amd import kitti_io as IO
    from tests.test_sor_gpu import _moving_frame
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lmono_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "map_build"])
    w, h, n = 320, 96, 2
    fx = fy = 185.0; cx = 156.5; cy = 47.25
    seq = tmp_path / "seq"; out = tmp_path / "out"
    os.makedirs(seq / "velodyne"); os.makedirs(seq / "image_bgr"); os.makedirs(out)
    M = CC.lidar_to_camera()
    mb = lmono_amd.MapBuilder(gpu_ctx, lmono_amd.Camera(w, h, fx, fy, cx, cy, 0, 0, 0, 0, 5, 0, 0), max_cloud_points=1 << 16)
    vm = lmono_amd.VoxelMap(gpu_ctx, leaf=0.1, max_voxels=1 << 18)
    qt = np.zeros((n, 7))
    for k in range(n):
        cloud, bgr, q, t = _moving_frame(k, w, h)
        IO.write_velodyne_bin(IO.velodyne_path(str(seq), k), cloud)
        (seq / "image_bgr" / ("%06d.bgr" % k)).write_bytes(bgr.tobytes())
        qt[k, :4] = q; qt[k, 4:] = t
        mb.associate(cloud, M, bgr, q, t)
        lmono_amd.VoxelMap.insert_frames(gpu_ctx, [vm], [mb])
    IO.write_trajectory(str(tmp_path / "traj.txt"), 50.0 + 0.1 * np.arange(n), qt)
    subprocess.check_call([os.path.join(host, "map_build"), str(seq), str(tmp_path / "traj.txt"), str(out), str(n), str(w), str(h),
                           repr(fx), repr(fy), repr(cx), repr(cy), "voxel=0.1:%d" % (1 << 18), "normals=0.3"])
    plain = IO.read_ply_binary(str(out / "rgb_map_voxel.ply"))
    pts, nrm = IO.read_ply_binary_normals(str(out / "rgb_map_voxel_normals.ply"))
    assert len(plain) > 100 and plain.tobytes() == vm.read().tobytes()
    assert pts[_by_point(pts)].tobytes() == plain[_by_point(plain)].tobytes()
    s = lmono_amd.SurfaceNormals(gpu_ctx, 1 << 18, radius=0.3)
    stats = s.compute_map(vm)
    cloud, (rec, _) = s.cloud(), s.read()
    cloud["bgra"] |= 0xff000000                                           # a PLY has no alpha: the reader sets it
    assert stats[2] > 100                                                  # the map is dense enough for normals
    assert R.canon(R.records_of(nrm)[_by_point(pts)]) == R.canon(R.records_of(rec)[_by_point(cloud)])
    for x in (s, vm, mb):
        x.close()
