"""scripts/icp_bench.py -- cost of the point-to-point ICP (lmono_icp_*) in the chain map builder -> aligner -> voxel map:
every builder's last world cloud (one 1241 x 376 frame of tests/colour_cases-style input: an S1 scan, a noise image) is aligned against a
leaf-0.1 voxel map of the same frame coloured under a pose a few centimetres off, for 1 and 64 streams.  Reports ms per call and per frame of
set_target_map and of the align (whole C-ABI calls, which end synchronised), the iterations run and the last iteration's pairs.  The share of
k_icp_step in the align's time is not measured here: it comes from a kernel trace of this script (one stream, few calls).
Prints one JSON line.  One process; run it under `timeout`.

  timeout 600 python scripts/icp_bench.py [--streams 1,64] [--calls 5] [--warmup 1] [--max-corr 0.5] [--max-iter 50] [--eps 1e-8] [--poll 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,64")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-corr", type=float, default=0.5)
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--eps", type=float, default=1e-8)
    ap.add_argument("--poll", type=int, default=2)
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
    out = {"image": [w, h], "max_corr": a.max_corr, "max_iter": a.max_iter, "eps": a.eps, "poll": a.poll, "leaf": 0.1, "runs": []}
    for n in [int(v) for v in a.streams.split(",")]:
        mbs = [lmono_amd.MapBuilder(ctx, cam, max_cloud_points=16, map_capacity_points=w * h) for _ in range(n)]
        als = [lmono_amd.CloudAligner(ctx, w * h, w * h, a.max_corr, a.max_iter, a.eps) for _ in range(n)]
        vms = [lmono_amd.VoxelMap(ctx, leaf=0.1, max_voxels=1 << 19) for _ in range(n)]
        for al in als:
            al.set_poll_interval(a.poll)
        q = np.array([[0.02, -0.03, np.sin(0.01 * s), 0.0] for s in range(n)]); q[:, 3] = np.sqrt(1 - (q[:, :3] ** 2).sum(1))
        t = np.array([[12.5 + 0.37 * s, -3.25, 0.75] for s in range(n)])
        cl = ([cloud.data_ptr()] * n, [cloud.shape[0]] * n, [M] * n, [image.data_ptr()] * n)
        # the map: the frame under the true pose; the frame to align: the same scan under a pose 3 cm and 0.2 degrees off
        lmono_amd.MapBuilder.associate_batch(ctx, mbs, *cl, q, t)
        lmono_amd.VoxelMap.insert_frames(ctx, vms, mbs)
        q2 = q.copy(); q2[:, 2] += 0.00175; q2 /= np.sqrt((q2 ** 2).sum(1))[:, None]
        t2 = t + np.array([0.03, -0.02, 0.01])
        for m in mbs:
            m.clear()
        pts = lmono_amd.MapBuilder.associate_batch(ctx, mbs, *cl, q2, t2)
        target, align = [], []
        for c in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            for al, vm in zip(als, vms):
                al.set_target_map(vm)
            t1 = time.perf_counter()
            stats = lmono_amd.CloudAligner.align_frames(als, mbs)
            t2_ = time.perf_counter()
            if c >= a.warmup:
                target.append((t1 - t0) * 1e3); align.append((t2_ - t1) * 1e3)
        run = {"streams": n, "points_per_frame": int(pts[0]), "target_points": int(stats[0][2]), "stats_stream0": [int(v) for v in stats[0]],
               "iterations": [int(v) for v in stats[:, 4]][:8], "status": [int(v) for v in stats[:, 5]][:8], "transform_stream0": als[0].transform().reshape(-1).tolist()}
        for name, ms in (("set_target_map", target), ("align", align)):
            med = float(np.median(ms))
            run[name] = {"ms_per_call_median": med, "ms_per_call_min": float(np.min(ms)), "ms_per_frame": med / n}
        out["runs"].append(run)
        for x in als + vms + mbs:
            x.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
