"""The host mirror's aligner (MapBuilder::setAligner) through the map_build program: filter -> align against the voxel map ->
insert, the first frame inserted as it is; the written map and the printed ICP lines equal the Python chain's over the same frames."""
import os
import subprocess

import numpy as np
import pytest

from tests import colour_cases as CC

pytestmark = pytest.mark.gpu


def test_cpp_map_build_aligns_in_front_of_the_voxel_map(gpu_ctx, tmp_path):
    """map_build ... sor=16:1.0 icp=0.5:20 voxel=0.1 writes rgb_map_voxel.ply, equal to the Python chain's read() over the same frames, and one
    ICP line per frame with the chain's iterations, status and pairs."""
    import lmono_amd
    from lmono_amd import kitti_io as IO
    from tests.test_sor_gpu import _moving_frame
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lmono_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "map_build"])
    w, h, n = 320, 96, 3
    fx = fy = 185.0; cx = 156.5; cy = 47.25
    seq = tmp_path / "seq"; out = tmp_path / "out"
    os.makedirs(seq / "velodyne"); os.makedirs(seq / "image_bgr"); os.makedirs(out)
    M = CC.lidar_to_camera()
    mb = lmono_amd.MapBuilder(gpu_ctx, lmono_amd.Camera(w, h, fx, fy, cx, cy, 0, 0, 0, 0, 5, 0, 0), max_cloud_points=1 << 16)
    f = lmono_amd.OutlierFilter(gpu_ctx, w * h, 16, 1.0)
    a = lmono_amd.CloudAligner(gpu_ctx, w * h, 1 << 18, 0.5, 20, 1e-8)
    vm, unaligned = (lmono_amd.VoxelMap(gpu_ctx, leaf=0.1, max_voxels=1 << 18) for _ in range(2))
    qt = np.zeros((n, 7))
    lines = []
    for k in range(n):
        cloud, bgr, q, t = _moving_frame(k, w, h)
        IO.write_velodyne_bin(IO.velodyne_path(str(seq), k), cloud)
        (seq / "image_bgr" / ("%06d.bgr" % k)).write_bytes(bgr.tobytes())
        qt[k, :4] = q; qt[k, 4:] = t
        mb.associate(cloud, M, bgr, q, t)
        lmono_amd.OutlierFilter.filter_frames([f], [mb])
        lmono_amd.VoxelMap.insert_filtered([unaligned], [f])
        if vm.size == 0:
            lmono_amd.VoxelMap.insert_filtered([vm], [f])
            lines.append("ICP %d iterations 0 status 3 N 0" % k)         # no align ran: what an align of nothing reports
        else:
            a.set_target_map(vm)
            st = lmono_amd.CloudAligner.align_filtered([a], [f])[0]
            lmono_amd.VoxelMap.insert_aligned([vm], [a])
            lines.append("ICP %d iterations %d status %d N %d" % (k, st[4], st[5], st[6]))
            assert st[4] >= 1 and st[6] > 100                            # the frames overlap: the align has pairs to work with
    IO.write_trajectory(str(tmp_path / "traj.txt"), 50.0 + 0.1 * np.arange(n), qt)
    text = subprocess.check_output([os.path.join(host, "map_build"), str(seq), str(tmp_path / "traj.txt"), str(out), str(n), str(w), str(h),
                                    repr(fx), repr(fy), repr(cx), repr(cy), "sor=16:1.0", "icp=0.5:20", "voxel=0.1:%d" % (1 << 18)], text=True)
    got = [ln.rsplit(" mse ", 1)[0] for ln in text.split("\n") if ln.startswith("ICP ")]
    assert got == lines
    ply = IO.read_ply_binary(str(out / "rgb_map_voxel.ply"))
    want = vm.read()
    assert len(want) > 100 and ply.tobytes() == want.tobytes() and want.tobytes() != unaligned.read().tobytes()
    for x in (a, f, vm, unaligned, mb):
        x.close()
