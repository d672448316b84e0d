"""scripts/voxel_compose_bench.py -- cost of composing submaps into a global voxel map (lmono_voxel_map_compose): 1 / 16 / 64
submaps (leaf 0.05) of one coloured S1 frame each (1241 x 376 image, as scripts/sor_bench.py), each at its own pose, composed under a small
rigid correction into a cleared 0.1 m map in ONE call, against the route the parent commit offers for the same voxels: read() every submap
to the host and insert() its points (which also loses the weights: every voxel counts as one point).  Whole calls timed on the host, median
of --calls after --warmup.  Also reports the distinct-key ratio: voxels new in the cleared destination / source voxels moved -- the share of
entries a workgroup table could NOT have merged even if it saw the whole call at once (an upper bound on the merging per 512-record tile).
With --compact every submap is shrunk to what it holds (shrink_to_fit) before the composes, as SubmapAtlas(compact_closed=True) leaves closed
submaps: the compose then scans tables of that size.  "submap_table_bytes" is the device memory of the submaps' tables either way.
Prints one JSON line.  One process; run it under `timeout`.

  timeout 600 python scripts/voxel_compose_bench.py [--submaps 1,16,64] [--calls 5] [--warmup 1] [--compact]"""
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
    ap.add_argument("--submaps", default="1,16,64")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--compact", action="store_true")
    a = ap.parse_args()
    import lmono_amd
    from tests import colour_cases as CC
    ctx = lmono_amd.Context(0)
    w, h = 1241, 376
    cam = lmono_amd.Camera(w, h, 718.856, 718.856, 607.1928, 185.2157, 0, 0, 0, 0, 5, 0, 0)
    M = CC.lidar_to_camera()
    cloud = CC.s1_scan(); image = CC.noise_image(h, w)
    mb = lmono_amd.MapBuilder(ctx, cam, max_cloud_points=len(cloud), map_capacity_points=w * h)
    out = {"image": [w, h], "leaf_sub": 0.05, "leaf": 0.1, "compact": a.compact, "runs": []}
    for n in [int(v) for v in a.submaps.split(",")]:
        subs, T = [], []
        for s in range(n):
            q = np.array([0.02, -0.03, np.sin(0.01 * s), 0.0]); q[3] = np.sqrt(1 - (q[:3] ** 2).sum())
            t = np.array([12.5 + 0.37 * s, -3.25, 0.75])
            mb.clear()
            mb.associate(cloud, M, image, q, t)
            sub = lmono_amd.VoxelMap(ctx, leaf=0.05, max_voxels=1 << 19)
            sub.insert_frame(mb)
            subs.append(sub)
            inserted = np.concatenate([t, q])
            corrected = np.concatenate([t + np.array([0.05 * s, -0.02 * s, 0.0]), q])
            T.append(lmono_amd.pose_delta(inserted, corrected))
        if a.compact:
            lmono_amd.VoxelMap.reserve_batch(subs, [max(sub.size, 1) for sub in subs])
        dst = lmono_amd.VoxelMap(ctx, leaf=0.1, max_voxels=1 << 22)
        compose, route, st = [], [], None
        for c in range(a.warmup + a.calls):
            dst.clear()
            t0 = time.perf_counter()
            st = dst.compose(subs, T, stats=True)
            t1 = time.perf_counter()
            if c >= a.warmup:
                compose.append((t1 - t0) * 1e3)
        composed_voxels = dst.size
        for c in range(a.warmup + a.calls):
            dst.clear()
            t0 = time.perf_counter()
            for sub in subs:
                dst.insert(sub.read())
            t1 = time.perf_counter()
            if c >= a.warmup:
                route.append((t1 - t0) * 1e3)
        run = {"submaps": n, "submap_table_bytes": 64 * sum(sub.capacity.slots for sub in subs),
               "source_voxels": int(st[0] + st[1]), "points": int(st[2] + st[3]), "voxels_composed": int(composed_voxels), "voxels_read_insert_untransformed": int(dst.size),
               "distinct_key_ratio": float(st[4]) / max(float(st[0]), 1.0),
               "compose": {"ms_per_call_median": float(np.median(compose)), "ms_per_call_min": float(np.min(compose))},
               "read_insert": {"ms_per_call_median": float(np.median(route)), "ms_per_call_min": float(np.min(route))}}
        out["runs"].append(run)
        for x in subs + [dst]:
            x.close()
    mb.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
