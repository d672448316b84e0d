"""scripts/normals_bench.py -- cost of the surface normals (lmono_normals_*): one 1241 x 376 colour frame (the frame of
scripts/icp_bench.py: an S1 scan, a noise image; every builder's last world cloud) through compute_frames for 1 stream at each radius and for 64
streams at the first radius, and compute_map over the leaf-0.1 voxel map of that frame at the map radius.  Whole C-ABI calls, which end
synchronised (grid build, k_nrm_compute, k_nrm_stats and the read-back of the stats), timed by the host clock.  Reports ms per call, stats[4]
(neighbours visited and accepted, the query point included), neighbours per second, and the bytes of accepted neighbour records (16 B each,
the least k_nrm_compute must fetch; the rejected candidates of the scanned cells come on top) per second against the HBM and L2 peaks of
MI355X.  A whole-call rate over a peak, not a kernel's share of peak: the kernel's own time comes from a kernel trace of this script.
Prints one JSON line.  One process; run it under `timeout`.

  timeout 600 python scripts/normals_bench.py [--radii 0.05,0.3] [--streams 64] [--map-radius 0.3] [--calls 5] [--warmup 1]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK, HBM_MEASURED, L2_PEAK = 8.0e12, 6.29e12, 34.5e12       # bytes / s: spec, float4 copy, aggregate L2
RECORD = 16                                                      # bytes of one neighbour record in the grid


def _rates(ms, stats, n_streams):
    med = float(np.median(ms))
    neigh = int(stats[:, 4].sum())
    per_s = neigh / (med * 1e-3)
    return {"ms_per_call_median": med, "ms_per_call_min": float(np.min(ms)), "ms_per_frame": med / n_streams, "neighbours": neigh,
            "neighbours_per_s": per_s, "neighbour_bytes_per_s": per_s * RECORD, "of_hbm_peak": per_s * RECORD / HBM_PEAK,
            "of_hbm_measured": per_s * RECORD / HBM_MEASURED, "of_l2_peak": per_s * RECORD / L2_PEAK,
            "stats_stream0": [int(v) for v in stats[0]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radii", default="0.05,0.3")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--map-radius", type=float, default=0.3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import torch
    import lmono_amd
    from tests import colour_cases as CC
    ctx = lmono_amd.Context(0)
    w, h = 1241, 376
    cam = lmono_amd.Camera(w, h, 718.856, 718.856, 607.1928, 185.2157, 0, 0, 0, 0, 5, 0, 0)
    M = CC.lidar_to_camera()
    cloud = torch.from_numpy(CC.s1_scan()).to("cuda:0"); image = torch.from_numpy(CC.noise_image(h, w)).to("cuda:0")
    torch.cuda.synchronize()
    radii = [float(v) for v in a.radii.split(",")]
    out = {"image": [w, h], "leaf": 0.1, "calls": a.calls, "warmup": a.warmup, "runs": []}

    def timed(fn):
        ms = []
        for c in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            stats = fn()
            if c >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms, np.asarray(stats).reshape(-1, 8)

    for n, rs in ((1, radii), (a.streams, radii[:1])):
        if n < 1:
            continue
        mbs = [lmono_amd.MapBuilder(ctx, cam, max_cloud_points=16, map_capacity_points=w * h) for _ in range(n)]
        q = np.array([[0.02, -0.03, np.sin(0.01 * s), 0.0] for s in range(n)]); q[:, 3] = np.sqrt(1 - (q[:, :3] ** 2).sum(1))
        t = np.array([[12.5 + 0.37 * s, -3.25, 0.75] for s in range(n)])
        pts = lmono_amd.MapBuilder.associate_batch(ctx, mbs, [cloud.data_ptr()] * n, [cloud.shape[0]] * n, [M] * n, [image.data_ptr()] * n, q, t)
        for r in rs:
            hs = [lmono_amd.SurfaceNormals(ctx, w * h, radius=r) for _ in range(n)]
            ms, stats = timed(lambda: lmono_amd.SurfaceNormals.compute_frames(hs, mbs, t.astype(np.float32)))
            out["runs"].append(dict({"what": "compute_frames", "streams": n, "radius": r, "points_per_frame": int(pts[0])}, **_rates(ms, stats, n)))
            for x in hs:
                x.close()
        if n == 1:
            vm = lmono_amd.VoxelMap(ctx, leaf=0.1, max_voxels=1 << 19)
            lmono_amd.VoxelMap.insert_frames(ctx, [vm], mbs)
            s = lmono_amd.SurfaceNormals(ctx, 1 << 19, radius=a.map_radius)
            ms, stats = timed(lambda: s.compute_map(vm))
            out["runs"].append(dict({"what": "compute_map", "streams": 1, "radius": a.map_radius, "voxels": int(vm.size)}, **_rates(ms, stats, 1)))
            s.close(); vm.close()
        for x in mbs:
            x.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
