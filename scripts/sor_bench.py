"""scripts/sor_bench.py -- cost of the statistical outlier removal (lmono_sor_filter_frames) in the chain map builder ->
filter -> voxel map: every builder's last world cloud (one 1241 x 376 frame of tests/colour_cases-style input: an S1 scan, a noise image)
goes through its own filter (k = 100, cell 0.1, 8 rings unless given) and the kept points into its own voxel map, for 1 and 64 streams.
Reports ms per call and per frame of the filter, of the colour frame in front of it and of the filtered insert behind it, the filter's
statistics, the mean number of rings a query scanned and the share of scored queries that took the general (radix select) path.  The share
of k_sor_query in the filter's time is not measured here: it comes from a kernel trace of this script (one stream, few calls).
Prints one JSON line.  One process; run it under `timeout`.

  timeout 600 python scripts/sor_bench.py [--streams 1,64] [--calls 5] [--warmup 1] [--k 100] [--mul 1.0] [--cell 0.1] [--rings 8]"""
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
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--mul", type=float, default=1.0)
    ap.add_argument("--cell", type=float, default=0.1)
    ap.add_argument("--rings", type=int, default=8)
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
    out = {"image": [w, h], "mean_k": a.k, "stddev_mul": a.mul, "cell": a.cell, "max_rings": a.rings, "runs": []}
    for n in [int(v) for v in a.streams.split(",")]:
        mbs = [lmono_amd.MapBuilder(ctx, cam, max_cloud_points=16, map_capacity_points=w * h) for _ in range(n)]
        fs = [lmono_amd.OutlierFilter(ctx, w * h, a.k, a.mul, a.cell, a.rings) for _ in range(n)]
        vms = [lmono_amd.VoxelMap(ctx, leaf=0.1, max_voxels=1 << 19) for _ in range(n)]
        q = np.array([[0.02, -0.03, np.sin(0.01 * s), 0.0] for s in range(n)]); q[:, 3] = np.sqrt(1 - (q[:, :3] ** 2).sum(1))
        t = np.array([[12.5 + 0.37 * s, -3.25, 0.75] for s in range(n)])
        args = ([cloud.data_ptr()] * n, [cloud.shape[0]] * n, [M] * n, [image.data_ptr()] * n, q, t)
        colour, filt, insert = [], [], []
        for c in range(a.warmup + a.calls):
            for m in mbs:
                m.clear()
            t0 = time.perf_counter()
            pts = lmono_amd.MapBuilder.associate_batch(ctx, mbs, *args)
            t1 = time.perf_counter()
            stats = lmono_amd.OutlierFilter.filter_frames(fs, mbs)
            t2 = time.perf_counter()
            lmono_amd.VoxelMap.insert_filtered(vms, fs)
            t3 = time.perf_counter()
            if c >= a.warmup:
                colour.append((t1 - t0) * 1e3); filt.append((t2 - t1) * 1e3); insert.append((t3 - t2) * 1e3)
        diag = np.array([f.diag() for f in fs])
        valid = float((stats[:, 0] - stats[:, 1]).sum())
        run = {"streams": n, "points_per_frame": int(pts[0]), "stats_stream0": [int(v) for v in stats[0]],
               "rings_per_query_mean": float(diag[:, 0].sum()) / max(valid, 1.0), "general_path_share_of_scored": float(diag[:, 1].sum()) / max(float(stats[:, 3].sum()), 1.0)}
        for name, ms in (("colour", colour), ("filter", filt), ("insert_filtered", insert)):
            med = float(np.median(ms))
            run[name] = {"ms_per_call_median": med, "ms_per_call_min": float(np.min(ms)), "ms_per_frame": med / n}
        out["runs"].append(run)
        for x in fs + vms + mbs:
            x.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
