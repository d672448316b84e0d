"""scripts/track_bench.py -- throughput of the device feature tracker (lmono_tracker_track_batch): frames/s for 1, 8, 64, 256
streams at 1241 x 376 with 150 points, images resident on the device, plus per-kernel times of one 64-stream frame from the
torch profiler's device events.  Prints one JSON line.  One process; run it under `timeout`; exits non-zero on any HIP error.

  timeout 300 python scripts/track_bench.py [--streams 1,8,64,256] [--frames 12] [--warmup 3] [--no-kernels] [--reject-f THR DIS]

--reject-f switches rejectWithF on in every stream (lmono_tracker_set_reject_f; k_trk_reject then shows among the kernels)."""
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
    ap.add_argument("--streams", default="1,8,64,256")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1241)
    ap.add_argument("--height", type=int, default=376)
    ap.add_argument("--max-cnt", type=int, default=150)
    ap.add_argument("--min-dist", type=int, default=30)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--reject-f", type=float, nargs=2, metavar=("THR", "DIS"))
    a = ap.parse_args()
    import torch
    import lmono_amd
    from workloads import s5
    w, h = a.width, a.height
    n_img = a.frames + a.warmup
    variants = [s5.Sequence(w, h, n_img, seed=20 + v, step=(2.0 + 0.5 * v, 0.5 * v - 0.5), margin=64).frames for v in range(4)]
    dev = [[torch.from_numpy(f).to("cuda:0") for f in seq] for seq in variants]       # 4 sequences shared by all streams (device resident)
    torch.cuda.synchronize()
    ctx = lmono_amd.Context(0)
    cam = lmono_amd.Camera(w, h, 718.856, 718.856, 607.1928, 185.2157, 0.0, 0.0, 0.0, 0.0, 5, 0, 0)
    out = {"bench": "track", "width": w, "height": h, "max_cnt": a.max_cnt, "min_dist": a.min_dist, "frames": a.frames, "warmup": a.warmup,
           "reject_f": a.reject_f, "runs": []}
    for n in [int(x) for x in a.streams.split(",")]:
        batch = lmono_amd.FeatureTrackerBatch(ctx, [cam] * n, a.max_cnt, a.min_dist,
                                              reject_f=dict(f_threshold=a.reject_f[0], f_dis=a.reject_f[1]) if a.reject_f else None)
        ms = []
        feats = 0
        for f in range(n_img):
            ptrs = [dev[s % 4][f].data_ptr() for s in range(n)]
            t0 = time.perf_counter()
            rec = batch.track([0.1 * f] * n, ptrs)                                        # synchronises before it returns
            dt = (time.perf_counter() - t0) * 1e3
            if f >= a.warmup:
                ms.append(dt); feats = sum(len(r) for r in rec)
        ms = np.array(ms)
        out["runs"].append({"streams": n, "ms_per_call_median": float(np.median(ms)), "ms_per_call_min": float(ms.min()), "ms_per_call_max": float(ms.max()),
                            "frames_per_s": float(n * 1e3 / np.median(ms)), "features_last_frame": int(feats)})
        if n == 64 and not a.no_kernels:
            from torch.profiler import ProfilerActivity, profile
            batch.reset()
            for f in range(2):
                batch.track([0.1 * f] * n, [dev[s % 4][f].data_ptr() for s in range(n)])
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                batch.track([0.2] * n, [dev[s % 4][2].data_ptr() for s in range(n)])
                torch.cuda.synchronize()
            kern = {}
            for e in prof.key_averages():
                if "k_trk_" in e.key:
                    name = e.key[e.key.index("k_trk_"):].split("(")[0]
                    name = name.split("E")[0] if e.key.startswith("_Z") else name
                    us = getattr(e, "device_time_total", None)
                    if us is None:
                        us = getattr(e, "cuda_time_total", 0.0)
                    kern[name] = kern.get(name, 0.0) + float(us)
            out["kernels_us_64_streams_steady_frame"] = kern
        batch.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
