"""scripts/voxel_map_bench.py -- throughput of the voxel-grid colour map's insert (lmono_voxel_map_insert_frames): points per
second and frames per second when every builder's last world cloud (one 1241 x 376 frame of tests/colour_cases-style input: an S1 scan, a
noise image) is folded into its own map, for 1 and 64 streams, with the workgroup's on-chip sum (the default) and in the plain form (one probe
and one set of adds per point, LMONO_VOXEL_FORM=0).  "first" is the insert into a cleared map (every voxel is claimed), "again" the steady
state (every voxel is found).  Also reports the input's distinct-key ratios (per frame and per workgroup tile), the colour frame's own time
and the bytes of atomic adds per second over the whole insert.  With --grow also: the same steady-state insert into maps whose growth is on
but never triggered ("summed_growth_on_*"), and the cost of one growth ("grow"): every map holds one frame and is shrunk to fit, then ONE
lmono_voxel_map_reserve call doubles all of them ("double") and one halves them again ("halve"); ns per occupied voxel and the bytes the two
launches move (old table read + new table cleared + records written) per second.  Prints one JSON line.  One process; run it under `timeout`.

  timeout 600 python scripts/voxel_map_bench.py [--streams 1,64] [--calls 20] [--warmup 3] [--leaf 0.1] [--grow]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def keys_of(p, leaf):
    inv = np.float32(1.0) / np.float32(leaf)
    t = np.stack([p["x"], p["y"], p["z"]], 1) * inv
    ok = ((t >= -1048576.0) & (t < 1048576.0)).all(1)
    i = np.floor(t[ok]).astype(np.int64) + (1 << 20)
    return (i[:, 2] << 42) | (i[:, 1] << 21) | i[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,64")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--leaf", type=float, default=0.1)
    ap.add_argument("--grow", action="store_true")
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
    out = {"image": [w, h], "leaf": a.leaf, "runs": []}
    for n in [int(v) for v in a.streams.split(",")]:
        mbs = [lmono_amd.MapBuilder(ctx, cam, max_cloud_points=16, map_capacity_points=w * h) for _ in range(n)]
        q = np.array([[0.02, -0.03, np.sin(0.01 * s), 0.0] for s in range(n)]); q[:, 3] = np.sqrt(1 - (q[:, :3] ** 2).sum(1))
        t = np.array([[12.5 + 0.37 * s, -3.25, 0.75] for s in range(n)])
        args = ([cloud.data_ptr()] * n, [cloud.shape[0]] * n, [M] * n, [image.data_ptr()] * n, q, t)
        colour_ms = []
        for c in range(a.warmup + a.calls):
            for m in mbs:
                m.clear()
            t0 = time.perf_counter()
            pts = lmono_amd.MapBuilder.associate_batch(ctx, mbs, *args)
            if c >= a.warmup:
                colour_ms.append((time.perf_counter() - t0) * 1e3)
        world = mbs[0].cloud(1)
        k = keys_of(world, a.leaf)
        tile = None
        run = {"streams": n, "points_per_frame": int(pts[0]), "points_per_call": int(pts.sum()), "colour_ms_per_call_median": float(np.median(colour_ms)),
               "distinct_keys_per_point_frame": len(np.unique(k)) / max(len(k), 1)}
        for form, limit in ((1, 0), (0, 0)) + (((1, 1 << 20),) if a.grow else ()):
            os.environ["LMONO_VOXEL_FORM"] = str(form)                  # read when a map is created
            vms = [lmono_amd.VoxelMap(ctx, leaf=a.leaf, max_voxels=1 << 19, grow_limit=limit) for _ in range(n)]
            tile = vms[0].TILE
            first, again = [], []
            for c in range(a.warmup + a.calls):
                for v in vms:
                    v.clear()
                t0 = time.perf_counter()
                stats = lmono_amd.VoxelMap.insert_frames(ctx, vms, mbs)
                t1 = time.perf_counter()
                lmono_amd.VoxelMap.insert_frames(ctx, vms, mbs)
                t2 = time.perf_counter()
                if c >= a.warmup:
                    first.append((t1 - t0) * 1e3); again.append((t2 - t1) * 1e3)
            per_tile = sum(len(np.unique(k[i:i + tile])) for i in range(0, len(k), tile)) / max(len(k), 1)
            entries = (per_tile if form else 1.0) * float(stats[:, 0].sum())
            for name, ms in (("first", first), ("again", again)):
                med = float(np.median(ms)) * 1e-3
                run["%s_%s" % ("summed_growth_on" if limit else ("plain", "summed")[form], name)] = {
                    "ms_per_call_median": med * 1e3, "ms_per_call_min": float(np.min(ms)), "points_per_s": float(stats[:, 0].sum()) / med, "frames_per_s": n / med,
                    "atomic_bytes_per_s_over_the_call": entries * 56.0 / med, "share_of_colour_frame": med * 1e3 / float(np.median(colour_ms))}
            run["voxels_per_frame"] = int(stats[0, 3]); run["distinct_keys_per_point_tile"] = per_tile; run["tile"] = tile
            if limit:                                                   # the maps hold two inserts of one frame each: the cost of one growth
                assert all(v.capacity.rehashes == 0 for v in vms)       # growth was on and never triggered
                size = [v.size for v in vms]
                lmono_amd.VoxelMap.reserve_batch(vms, size)
                double, halve = [], []
                for c in range(a.warmup + a.calls):
                    t0 = time.perf_counter()
                    lmono_amd.VoxelMap.reserve_batch(vms, [2 * v for v in size])
                    t1 = time.perf_counter()
                    slots2 = sum(v.capacity.slots for v in vms)
                    t2 = time.perf_counter()
                    lmono_amd.VoxelMap.reserve_batch(vms, size)
                    t3 = time.perf_counter()
                    if c >= a.warmup:
                        double.append((t1 - t0) * 1e3); halve.append((t3 - t2) * 1e3)
                slots1 = sum(v.capacity.slots for v in vms)
                run["grow"] = {"voxels_per_map": size[0], "slots_per_map": [vms[0].capacity.slots, slots2 // n]}
                for name, ms, rd, wr in (("double", double, slots1, slots2), ("halve", halve, slots2, slots1)):
                    med = float(np.median(ms)) * 1e-3
                    moved = 64.0 * (rd + wr + 1 * n + sum(size))        # old tables read, new tables (+ counter rows) cleared, records written
                    run["grow"][name] = {"ms_per_call_median": med * 1e3, "ms_per_call_min": float(np.min(ms)), "ns_per_voxel": med * 1e9 / sum(size),
                                         "bytes_moved": moved, "bytes_per_s_over_the_call": moved / med}
            for v in vms:
                v.close()
        os.environ.pop("LMONO_VOXEL_FORM", None)
        out["runs"].append(run)
        for m in mbs:
            m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
