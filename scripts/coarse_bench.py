"""scripts/coarse_bench.py -- cost of the FPFH descriptors (lmono_fpfh_*) and of the sample-consensus alignment (lmono_sacia_*,
DESIGN.md 6c-8): one 1241 x 376 colour frame (the frame of
scripts/normals_bench.py: an S1 scan, a noise image; every builder's last world cloud) with its normals, keypoints from a voxel map of that frame
at a coarse leaf (one point per occupied voxel, VoxelMap.read()), through FpfhDescriptors.compute for 1 stream at each radius and through
compute_batch for 64 streams at the first radius.  Whole C-ABI calls, which end synchronised (the keypoints' upload, the grid build, k_fpfh_clear,
k_fpfh_mark, k_fpfh_spfh, k_fpfh_weight and the read-back of the stats), timed by the host clock: median of --calls after --warmup.  Reports ms per
call and the call's stats.  Then CoarseAligner.align at --hyps hypotheses (30 is the reference's nr_iters) on the one-stream descriptors of the first
radius, the frame against itself: source and target are the same keypoints, which costs what two frames with as many keypoints cost (the read of
both sides' keypoints and flags, k_sacia_cand, k_sacia_hyp, k_sacia_best, the read-back).  Prints one JSON line.  One process; run it
under `timeout`.

  timeout 600 python scripts/coarse_bench.py [--radii 0.05,0.3] [--streams 64] [--hyps 30,1024,16384] [--keypoint-leaf 1.0] [--calls 5] [--warmup 1]"""
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
    ap.add_argument("--radii", default="0.05,0.3")
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--hyps", default="30,1024,16384")
    ap.add_argument("--keypoint-leaf", type=float, default=1.0)
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
    out = {"image": [w, h], "keypoint_leaf": a.keypoint_leaf, "calls": a.calls, "warmup": a.warmup, "runs": []}

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
        kps = []
        for mb in mbs:
            vm = lmono_amd.VoxelMap(ctx, leaf=a.keypoint_leaf, max_voxels=1 << 16)
            lmono_amd.VoxelMap.insert_frames(ctx, [vm], [mb])
            v = vm.read()
            kps.append(np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32)[:4096])
            vm.close()
        for r in rs:
            ns = [lmono_amd.SurfaceNormals(ctx, int(pts[s]), radius=r) for s in range(n)]
            lmono_amd.SurfaceNormals.compute_frames(ns, mbs, t.astype(np.float32))
            fs = [lmono_amd.FpfhDescriptors(ctx, int(pts[s]), 4096, radius=r) for s in range(n)]
            if n == 1:
                ms, stats = timed(lambda: fs[0].compute(ns[0], kps[0]))
            else:
                ms, stats = timed(lambda: lmono_amd.FpfhDescriptors.compute_batch(fs, ns, kps))
            med = float(np.median(ms))
            out["runs"].append({"what": "compute" if n == 1 else "compute_batch", "streams": n, "radius": r, "points_per_frame": int(pts[0]),
                                "keypoints_stream0": int(len(kps[0])), "ms_per_call_median": med, "ms_per_call_min": float(np.min(ms)), "ms_per_frame": med / n,
                                "pairs": int(stats[:, 4].sum()), "pairs_per_s": int(stats[:, 4].sum()) / (med * 1e-3), "stats_stream0": [int(v) for v in stats[0]]})
            if n == 1 and r == radii[0]:
                for nh in [int(v) for v in a.hyps.split(",") if v]:
                    al = lmono_amd.CoarseAligner(ctx, n_hyp=nh)
                    ms, st = timed(lambda: al.align(fs[0], fs[0]))
                    out["runs"].append({"what": "align", "n_hyp": nh, "radius": r, "usable_keypoints": int(st[0, 5]), "ms_per_call_median": float(np.median(ms)),
                                        "ms_per_call_min": float(np.min(ms)), "stats": [int(v) for v in st[0]]})
                    al.close()
            for x in fs + ns:
                x.close()
        for x in mbs:
            x.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
